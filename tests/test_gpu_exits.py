"""Exit lists (wost_exits_walk & co.; include/wost.h "Exit lists"): walk once, apply any Dirichlet data and its adjoint.

Every check stands on something outside the code under test: a record pushed through the numpy emulation (exits_emulation.py)
has to give the very number the library's own point solve gives for that walk, with the handle's colours and with any other
(a fresh handle made with them); the sums over a point's walks are compared with the emulation's fp64 ones within the bounds
derived in exits_emulation.py; and a harmonic linear function anchors the whole against the analytic solution.

Scenes carry random Dirichlet colours that differ per vertex and per side and a dirichlet_intensity of 1.25, so a wrong
primitive, side, weight or a forgotten factor shows.  Frame 16 x 16 (256 walks per launch), S = 8, max_depth = 32, eps = 1e-3.

Mutation check (run once on scratch copies of the library, not part of the suite; all 40 cases pass on the library as it is):
the side offset flipped in the apply and adjoint kernels, and uv and 1 - uv swapped in them, each fail 13 cases, among them
test_other_data_match_a_fresh_handle_made_with_them (all three scenes), test_adjoint_against_the_fp64_scatter_and_the_dot_product_identity
(all three) and test_vertices_nobody_exits_at_get_exactly_zero; base taken after the Dirichlet add in the 2-D walk kernel fails
18, among them every 2-D case of test_replay_per_walk_bit_for_bit and the 2-D analytic anchor."""
import numpy as np
import pytest

import exits_emulation as xe
from conftest import box_problem, cube_scene3
from test_gpu_parity import _integrator, _with_source
from test_gpu_points import COUNTERS, _it3, _mixed_box

pytestmark = pytest.mark.gpu

S, DEPTH, EPS, BASE, WIDTH, FRAME = 8, 32, 1e-3, 3000, 16, 16
INTENSITY = 1.25


def _colors(n_verts, seed):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, size=(n_verts, 6)).astype(np.float32)


def _scene(kind, colors=None):
    """-> (dim, scene, prims, n_verts); the scene carries `colors` (default: the random set of seed 100)"""
    if kind == "cube":
        sd = cube_scene3(n=3, d_faces=(0, 1, 4, 5), n_faces=(2, 3), value=lambda x, y, z: x + z)
        sd["d_colors"] = _colors(len(sd["d_verts"]), 100) if colors is None else np.ascontiguousarray(colors, np.float32)
        sd["dirichlet_intensity"] = INTENSITY
        return 3, sd, sd["d_tris"], len(sd["d_verts"])
    p = {"mixed": _mixed_box, "source": lambda: _with_source(_mixed_box(), 0.0, 1.0),
         "dirichlet": lambda: box_problem(value=lambda x, y: 1.0)}[kind]()
    p.d_colors = _colors(len(p.d_verts), 100) if colors is None else np.ascontiguousarray(colors, np.float32)
    p.dirichlet_intensity = INTENSITY
    return 2, p, p.d_segs, len(p.d_verts)


def _make(dim, scene, spp=1, depth=DEPTH, frame=FRAME):
    return _integrator(scene, frame, frame, spp, depth, EPS) if dim == 2 else _it3(scene, frame, frame, spp, depth, EPS)


def _points(dim):
    pts = np.random.default_rng(7).uniform(-0.25, 1.25, size=(200, dim)).astype(np.float32)
    pts[0, :2] = (0.5, 0.0)           # on the Dirichlet boundary
    pts[1, :2] = (0.5, 0.0005)        # inside the shell: absorbed at depth 0
    pts[2, :2] = (0.97, 0.5)          # next to the Neumann side
    pts[3, :2] = (300.0, -200.0)      # the far query: the scan by the wave
    if dim == 3:
        pts[:4, 2] = (0.5, 0.5, 0.5, 40.0)
        pts[0] = (0.0, 0.5, 0.5)      # on the face x = 0
        pts[1] = (0.0005, 0.4, 0.6)   # inside its shell
    return pts


def _single_walks(it, pts, S_, base, width):
    """the library's own answer for every walk of the list: one sample at point i on the stream of pixel base + i * S + s"""
    field = it.solve_points(np.repeat(pts, S_, axis=0), base, width)
    return field.reshape(len(pts), S_, 3), dict(it.last_stats)


def _walk(it, pts, S_=S, base=BASE, width=WIDTH):
    stats = it.exits_walk(pts, S_, base, width)
    assert it.exits_done == (len(pts), S_)
    rec = it.exits_records()
    assert rec["prim"].shape == (len(pts), S_) and rec["uv"].shape == (len(pts), S_, pts.shape[1] - 1) and rec["base"].shape == (len(pts), S_, 3)
    return rec, dict(stats)


def _same_records(a, b, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k], equal_nan=True) for k in ("prim", "uv", "side", "thp", "base"))


# ---- 1. / 5. replay per walk, bit for bit; record sanity ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 200])
@pytest.mark.parametrize("kind", ["mixed", "source", "dirichlet", "cube"])
def test_replay_per_walk_bit_for_bit(kind, n):
    """a 16 x 16 frame holds 32 points of 8 walks per launch: a part of a launch, one point short, a launch, one more, seven"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:n]
    it = _make(dim, scene)
    rec, stats = _walk(it, pts)
    want, want_stats = _single_walks(it, pts, S, BASE, WIDTH)
    it.close()
    colors = scene.d_colors if dim == 2 else scene["d_colors"]
    W = xe.walk_values(rec, colors, prims, INTENSITY, dim)
    assert W.dtype == np.float32 and np.array_equal(W, want), float(np.abs(W - want).max())
    for c in COUNTERS:
        assert stats[c] == want_stats[c], (c, stats[c], want_stats[c])
    assert stats["walks_started"] == n * S and stats["kernel_launches"] == -(-n * S // (FRAME * FRAME))
    # record sanity
    hit = rec["prim"] >= 0
    assert int(hit.sum()) == stats["walks_absorbed"] and np.all(rec["prim"][~hit] == -1) and np.all(rec["prim"] < len(prims))
    uv = rec["uv"][hit]
    assert np.all(uv > 0) and np.all(uv.sum(-1) < 1)
    assert np.all(np.isin(rec["side"], (-1, 0, 1))) and np.all(rec["uv"][~hit] == 0) and np.all(rec["side"][~hit] == 0)
    assert np.all(np.isfinite(rec["thp"])) and np.all(np.isfinite(rec["base"]))
    if n >= 4:
        assert hit[1].all()                                           # the point in the shell
        assert np.all(np.isfinite(W[3]))                              # the far point walks
    if n == 200:
        assert 0 < stats["walks_absorbed"] < n * S
        if kind != "dirichlet":
            assert stats["walks_truncated"] > 0 and stats["neumann_hits"] > 0
        assert np.any(rec["side"][hit] < 0) and np.any(rec["side"][hit] > 0)      # points on both sides of the boundary
        if kind in ("mixed", "source"):
            assert np.any(rec["base"][hit] != 0)                      # what the emissive Neumann sides and the source added


# ---- 2. other data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "source", "cube"])
def test_other_data_match_a_fresh_handle_made_with_them(kind):
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    sets = np.stack([_colors(n_verts, 200 + k) for k in range(3)])
    it = _make(dim, scene)
    rec, _ = _walk(it, pts)
    field, se = it.exits_apply(sets, want_stderr=True)
    only_field = it.exits_apply(sets)
    it.close()
    assert field.shape == se.shape == (3, 70, 3) and field.dtype == se.dtype == np.float32 and np.array_equal(field, only_field)
    emu = xe.apply(rec, sets, prims, INTENSITY, dim)
    for k in range(3):
        fresh = _make(dim, _scene(kind, sets[k])[1])
        want, _ = _single_walks(fresh, pts, S, BASE, WIDTH)
        fresh.close()
        assert np.array_equal(emu["W"][k], want), (k, float(np.abs(emu["W"][k] - want).max()))
    err = np.abs(field.astype(np.float64) - emu["mean"])
    print("field: max error / bound %.3f" % float((err / np.maximum(xe.field_bound(emu), 1e-300)).max()))
    assert np.all(err <= xe.field_bound(emu))
    # the library's fp32 standard error against the emulation's fp64 one (a point whose walks all agree: exactly 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(se.astype(np.float64) - emu["stderr64"]) / emu["stderr64"]
    rel = np.where(emu["stderr64"] > 0, rel, np.abs(se))
    print("stderr: max relative error / bound %.3f" % float(rel.max() / xe.stderr_rel_bound(S)))
    assert np.all(rel <= xe.stderr_rel_bound(S)), float(rel.max())
    assert np.any(field[0] != field[1]) and np.all(np.isfinite(field))


def test_one_walk_per_point_has_an_infinite_standard_error():
    dim, scene, prims, n_verts = _scene("mixed")
    it = _make(dim, scene)
    pts = _points(2)[:40]
    rec, _ = _walk(it, pts, S_=1)
    field, se = it.exits_apply(scene.d_colors, want_stderr=True)
    it.close()
    assert np.all(np.isposinf(se)) and np.array_equal(field[0], xe.walk_values(rec, scene.d_colors, prims, INTENSITY, 2)[:, 0])


# ---- 3. adjoint --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "source", "cube"])
def test_adjoint_against_the_fp64_scatter_and_the_dot_product_identity(kind):
    """identity: field is affine in the colours, so on the difference of two sets  sum (field_A - field_B) v = sum (c_A - c_B)
    adjoint(v).  The library's numbers are fp32: a field entry is rounded once (2^-24) from walks that each carry at most five
    fp32 roundings of numbers no larger than |col| + |base| <= 2 max(|W|, |base|); an adjoint entry is rounded once.  Hence
    |lhs - rhs| <= 2^-24 [ sum |v| (|field_A| + |field_B| + 10 (m_A + m_B)) + sum |c_A - c_B| |adjoint| ] with m = the mean
    over a point's walks of max(|W|, |base|), plus the fp64 rounding of the two sums themselves"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    rng = np.random.default_rng(17)
    K = 2
    v = rng.normal(size=(K, len(pts), 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, stats = _walk(it, pts)
    got = it.exits_adjoint(v)
    again = it.exits_adjoint(v)
    cA, cB = np.stack([_colors(n_verts, 300 + k) for k in range(K)]), np.stack([_colors(n_verts, 400 + k) for k in range(K)])
    fA, fB = it.exits_apply(cA), it.exits_apply(cB)
    it.close()
    assert got.shape == (K, n_verts, 6) and got.dtype == np.float32
    emu = xe.adjoint(rec, v, prims, n_verts, INTENSITY, dim)
    for out in (got, again):
        err = np.abs(out.astype(np.float64) - emu["value"])
        assert np.all(err <= xe.adjoint_bound(emu)), float((err - xe.adjoint_bound(emu)).max())
        assert np.all(out[emu["terms"] == 0] == 0.0)
    assert int(emu["terms"].sum()) == stats["walks_absorbed"] * dim * 3 * K and np.any(emu["terms"] > 1)
    eA, eB = xe.apply(rec, cA, prims, INTENSITY, dim), xe.apply(rec, cB, prims, INTENSITY, dim)
    m = sum(np.maximum(np.abs(e["W"]), np.abs(rec["base"])[None]).astype(np.float64).mean(2) for e in (eA, eB))
    v64 = v.astype(np.float64)
    lhs = float(((fA.astype(np.float64) - fB.astype(np.float64)) * v64).sum())
    rhs = float(((cA.astype(np.float64) - cB.astype(np.float64)) * got.astype(np.float64)).sum())
    tol = 2.0 ** -24 * float((np.abs(v64) * (np.abs(fA) + np.abs(fB) + 10.0 * m)).sum() + (np.abs(cA - cB) * np.abs(got)).sum())
    print("identity: lhs %.9g rhs %.9g, |difference| / tolerance %.3f" % (lhs, rhs, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol * (1.0 + 1e-6)
    assert abs(lhs) > 1e3 * tol      # (the identity is not met by two numbers that are small)


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_vertices_nobody_exits_at_get_exactly_zero(kind):
    """three points of two walks: at most 6 dim of the entries of a channel can be touched, far fewer than there are, and the
    point inside the shell is absorbed at once, so some are"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:3]
    v = np.random.default_rng(19).normal(size=(1, 3, 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, stats = _walk(it, pts, S_=2)
    got = it.exits_adjoint(v)
    it.close()
    emu = xe.adjoint(rec, v, prims, n_verts, INTENSITY, dim)
    assert 6 * dim < n_verts * 2 and stats["walks_absorbed"] >= 2
    assert np.any(emu["terms"] == 0) and np.any(emu["terms"] > 0)
    assert np.all(got[emu["terms"] == 0] == 0.0) and np.all(got[emu["terms"] > 0] != 0.0)
    assert np.all(np.abs(got.astype(np.float64) - emu["value"]) <= xe.adjoint_bound(emu))


# ---- 4. the analytic anchor --------------------------------------------------------------------------------------------------
LIN = dict(S=256, base=4096, width=64, frame=32)


def _oracle_depth(oracle, dim, sd, pts):
    """the smallest of 64, 128, 256, 512 at which the oracle truncates none of the list's walks: all pixels of a probe of scale
    0 at p evaluate p, and pixel k walks on stream k, so one oracle solve per point takes its S single-sample walks"""
    for depth in (64, 128, 256, 512):
        truncated = 0
        for i, p in enumerate(pts):
            sd = dict(sd)
            k0 = LIN["base"] + i * LIN["S"]
            height = -(-(k0 + LIN["S"]) // LIN["width"])
            if dim == 2:
                sd["probe"] = (0.0, float(p[0]), float(p[1]), 0.0, 1.0)
                r = oracle.solve(sd, LIN["width"], height, 1, depth, EPS, pixel_begin=k0, pixel_end=k0 + LIN["S"], threads=4)
            else:
                sd["probe"] = (0.0, tuple(float(x) for x in p), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))
                r = oracle.solve3(sd, LIN["width"], height, 1, depth, EPS, pixel_begin=k0, pixel_end=k0 + LIN["S"], threads=4)
            truncated += int(r["walks_truncated"])
        if truncated == 0:
            return depth
    raise AssertionError("the oracle truncates walks at every depth tried")


@pytest.mark.parametrize("dim", [2, 3])
def test_the_analytic_anchor_of_linear_data(oracle, dim):
    """u = a x + b is harmonic, walk on spheres is exact in expectation for it, and the exit lies within eps of its projection:
    |field - (a x + b)| <= 4 stderr + |a| eps at interior points, for two sets (a, b) applied to ONE walk.  The uniform walk
    keeps thp = 1 exactly in every scene (1 / pdf / alpha / 2 pi is 1.0f, tests/test_oracle_units.py), so neither this anchor
    nor the replay can see a missing thp: the factor is recorded and applied because the step has it; weights swapped on a
    segment move an exit's value by up to |a| / 8 (the segments are 1 / 8 long), its mean by about |a| / 16 -- several times the
    bound, which is about 4 |a| 0.29 / 16 = |a| / 14 at the centre and smaller near the boundary -- and a flipped side offset
    reads the same colours here and is caught by the replay instead"""
    ab = [(2.0, 1.0), (-0.75, 0.25)]
    if dim == 2:
        scene = box_problem(value=lambda x, y: 1.0)
        verts, n = scene.d_verts, 24
    else:
        scene = cube_scene3(n=4, value=lambda x, y, z: 1.0)
        verts, n = scene["d_verts"], 16
    pts = np.random.default_rng(3).uniform(0.1, 0.9, size=(n, dim)).astype(np.float32)
    depth = _oracle_depth(oracle, dim, scene.as_dict() if dim == 2 else scene, pts)
    sets = np.stack([np.repeat((np.float32(a) * verts[:, 0] + np.float32(b))[:, None], 6, axis=1) for a, b in ab]).astype(np.float32)
    it = _make(dim, scene, depth=depth, frame=LIN["frame"])
    stats = it.exits_walk(pts, LIN["S"], LIN["base"], LIN["width"])
    field, se = it.exits_apply(sets, want_stderr=True)
    it.close()
    assert stats["walks_truncated"] == 0 and stats["walks_absorbed"] == n * LIN["S"]
    for k, (a, b) in enumerate(ab):
        truth = a * pts[:, 0].astype(np.float64) + b
        err = np.abs(field[k].astype(np.float64) - truth[:, None])
        bound = 4.0 * se[k].astype(np.float64) + abs(a) * EPS
        print("dim %d set %d depth %d: max |error| / bound %.3f" % (dim, k, depth, float((err / bound).max())))
        assert np.all(err <= bound), float((err / bound).max())
        assert np.all(se[k] > 0) and np.array_equal(field[k][:, 0], field[k][:, 1])


# ---- 6. a cut list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_a_cut_list_gives_the_same_records_and_field(kind):
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)
    sets = np.stack([_colors(n_verts, 500 + k) for k in range(2)])
    v = np.random.default_rng(23).normal(size=(2, len(pts), 3)).astype(np.float32)
    it = _make(dim, scene)
    whole, _ = _walk(it, pts)
    field, adj = it.exits_apply(sets), it.exits_adjoint(v)
    head, _ = _walk(it, pts[:77])
    field_head, adj_head = it.exits_apply(sets), it.exits_adjoint(v[:, :77])
    tail, _ = _walk(it, pts[77:], base=BASE + 77 * S)
    field_tail, adj_tail = it.exits_apply(sets), it.exits_adjoint(v[:, 77:])
    it.close()
    assert _same_records(whole, head, slice(0, 77)) and _same_records(whole, tail, slice(77, None))
    assert np.array_equal(field[:, :77], field_head) and np.array_equal(field[:, 77:], field_tail)
    # The adjoint of the whole list is the sum of the two parts': each entry's terms are split over them.  Bound 3 holds each
    # of the THREE results to its own exact sum -- its M 2^-52 sum|terms| and one rounding, 2^-24 of ITS value -- so the
    # difference is held to the sum of the three.  The whole list's bound alone cannot hold: where the head's and the tail's
    # entries cancel, |head| and |tail| are large beside |whole|, and their two roundings to fp32 (2^-24 |head|, 2^-24 |tail|)
    # exceed 2^-24 |whole| however exactly every sum was taken.
    bound = sum(xe.adjoint_bound(xe.adjoint(r, d, prims, n_verts, INTENSITY, dim))
                for r, d in ((whole, v), (head, v[:, :77]), (tail, v[:, 77:])))
    assert np.all(np.abs(adj.astype(np.float64) - (adj_head.astype(np.float64) + adj_tail.astype(np.float64))) <= bound)


# ---- 7. the device forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_device_arrays_on_the_callers_stream(kind):
    import torch
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    n, K = len(pts), 2
    sets = np.stack([_colors(n_verts, 600 + k) for k in range(K)])
    v = np.random.default_rng(29).normal(size=(K, n, 3)).astype(np.float32)
    it = _make(dim, scene)
    host_rec, host_stats = _walk(it, pts)
    host_field, host_se = it.exits_apply(sets, want_stderr=True)
    emu = xe.adjoint(host_rec, v, prims, n_verts, INTENSITY, dim)
    stream = torch.cuda.current_stream().cuda_stream

    def on_device(p):
        d_pts = torch.from_numpy(p).cuda()
        stats = it.exits_walk_dev(d_pts.data_ptr(), n, S, stream, BASE, WIDTH)
        rec = it.exits_records()
        d_sets, d_v = torch.from_numpy(sets).cuda(), torch.from_numpy(v).cuda()
        field, se = (torch.full((K, n, 3), -1.0, dtype=torch.float32, device="cuda") for _ in range(2))
        adj = torch.full((K, n_verts, 6), -1.0, dtype=torch.float32, device="cuda")
        it.exits_apply_dev(d_sets.data_ptr(), K, field.data_ptr(), stream, se.data_ptr())
        it.exits_adjoint_dev(d_v.data_ptr(), K, adj.data_ptr(), stream)
        only = torch.full((K, n, 3), -1.0, dtype=torch.float32, device="cuda")
        it.exits_apply_dev(d_sets.data_ptr(), K, only.data_ptr(), None)
        assert np.array_equal(only.cpu().numpy(), field.cpu().numpy(), equal_nan=True)
        return rec, stats, field.cpu().numpy(), se.cpu().numpy(), adj.cpu().numpy()

    rec, stats, field, se, adj = on_device(pts)
    assert _same_records(host_rec, rec) and np.array_equal(field, host_field) and np.array_equal(se, host_se)
    for c in COUNTERS:
        assert stats[c] == host_stats[c], c
    assert np.all(np.abs(adj.astype(np.float64) - emu["value"]) <= xe.adjoint_bound(emu))
    # a NaN coordinate: that point is never walked, its field is NaN; its neighbours keep their bits
    bad = pts.copy()
    bad[37, 1] = np.nan
    rec, stats, field, se, adj = on_device(bad)
    rest = np.arange(n) != 37
    assert np.all(rec["prim"][37] == -1) and np.all(np.isnan(rec["thp"][37])) and np.all(np.isnan(rec["base"][37]))
    assert np.all(np.isnan(field[:, 37])) and np.array_equal(field[:, rest], host_field[:, rest]) and np.array_equal(se[:, rest], host_se[:, rest])
    assert all(np.array_equal(rec[k][rest], host_rec[k][rest]) for k in rec)
    assert stats["walks_started"] == (n - 1) * S
    assert np.all(np.isfinite(adj))      # (a point that is not walked exits nowhere)
    it.close()


# ---- 8. neighbours -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_the_list_and_its_neighbours_leave_one_another_alone(kind):
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
            rec, _ = _walk(it, pts)
            mine = [rec, it.exits_apply(sets)]
        out.append(it.solve_points(listed, 9, 16))
        it.solve_more(3)
        out.append(it.solution.copy())
        it.points_carry(listed, 9, 16)
        out.append(it.points_more(2))
        g = it.solve_gradient_points(listed[:20], 500, 1000, 32)
        out += [g["grad"], g["field"]]
        if dim == 2:
            it.set_option("spp", 5)      # (the 3-D handle has no such option)
        it.solve()
        out.append(it.solution.copy())
        it.solve_more(2)
        out.append(it.solution.copy())
        if with_list:
            assert it.exits_done == (len(pts), S)
            assert _same_records(mine[0], it.exits_records()) and np.array_equal(mine[1], it.exits_apply(sets))
        it.close()
        return out

    plain, mixed = run(False), run(True)
    assert np.any(plain[0] != 0) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, mixed))


# ---- 9. refusals that need the handle ------------------------------------------------------------------------------------------
WOST_ERR_INVALID, WOST_ERR_UNSUPPORTED = -1, -3


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_refusals_that_need_the_handle(kind):
    from elaina_amd import capi
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:10]
    it = _make(dim, scene)
    sets = _colors(n_verts, 800)[None]
    with pytest.raises(capi.WostError, match="no exit list is bound"):
        it.exits_apply(sets)
    with pytest.raises(capi.WostError, match="no exit list is bound"):
        it.exits_records()
    first, _ = _walk(it, pts)
    field = it.exits_apply(sets)
    # a refused walk leaves the list as it was
    with pytest.raises(capi.WostError, match="walk_seed_base"):
        it.exits_walk(pts[:3], S, -1, WIDTH)
    bad = pts.copy()
    bad[4, 0] = np.inf
    with pytest.raises(capi.WostError, match="point 4 "):
        it.exits_walk(bad, S, BASE, WIDTH)
    assert it.exits_done == (10, S) and _same_records(first, it.exits_records()) and np.array_equal(field, it.exits_apply(sets))
    # a new walk replaces it
    second, _ = _walk(it, pts[:6], S_=3, base=BASE + 1)
    assert it.exits_done == (6, 3) and it.exits_apply(sets).shape == (1, 6, 3)
    assert not np.array_equal(second["uv"], first["uv"][:6, :3])      # (other streams: other exits)
    # n = 0 releases it
    it.exits_walk(pts[:0], S, BASE, WIDTH)
    assert it.exits_done == (0, 0)
    with pytest.raises(capi.WostError, match="no exit list is bound"):
        it.exits_apply(sets)
    d, out = np.zeros((1, 6, 3), np.float32), np.full((1, n_verts, 6), -1.0, np.float32)
    assert getattr(it.lib, it._prefix + "exits_adjoint")(it._handle, capi._fp(d), 1, capi._fp(out)) == WOST_ERR_INVALID
    assert b"no exit list is bound" in it.lib.wost_last_error() and np.all(out == -1.0)
    it.close()


def test_the_adjoint_needs_a_dirichlet_mesh():
    """a scene of Neumann sides only: the walks end by truncation, every record says so, apply gives the bases -- and there are no
    colours to differentiate by"""
    import ctypes as C
    from elaina_amd import capi
    p = box_problem(d_sides=(), n_sides=(0, 1, 2, 3), flux=lambda x, y, s: 0.5)
    it = _integrator(p, FRAME, FRAME, 1, DEPTH, EPS)
    pts = np.random.default_rng(2).uniform(0.2, 0.8, size=(12, 2)).astype(np.float32)
    rec, stats = _walk(it, pts)
    want, want_stats = _single_walks(it, pts, S, BASE, WIDTH)
    assert np.all(rec["prim"] == -1) and np.array_equal(rec["base"], want) and stats["walks_absorbed"] == 0
    for c in COUNTERS:
        assert stats[c] == want_stats[c], c
    colors, field = np.zeros(1, np.float32), np.full((1, 12, 3), -1.0, np.float32)
    assert it.lib.wost_exits_apply(it._handle, capi._fp(colors), 1, capi._fp(field), None) == 0
    # (every record is its base: the emulation applies unchanged, on a mesh of one unused segment)
    emu = xe.apply(rec, np.zeros((1, 2, 6), np.float32), np.zeros((1, 2), np.int32), 1.0, 2)
    assert np.array_equal(emu["W"][0], want) and np.all(np.abs(field.astype(np.float64) - emu["mean"]) <= xe.field_bound(emu))
    out = np.full(6, -1.0, np.float32)
    assert it.lib.wost_exits_adjoint(it._handle, capi._fp(field), 1, capi._fp(out)) == WOST_ERR_UNSUPPORTED
    assert b"Dirichlet" in it.lib.wost_last_error() and np.all(out == -1.0)
    it.close()
