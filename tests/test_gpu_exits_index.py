"""The index of an exit list and the ordered adjoints (wost_exits_index & co.; include/wost.h "Exit lists: the index and the
ordered adjoint"): the adjoints as gathers in a stated summation order, so that dcolors is the same bits on every run.

Every check stands on something outside the code under test: the index is rebuilt in numpy from exits_records() and compared
integer for integer; the ordered results are compared BIT FOR BIT with exits_index_emulation.py, which adds the float64 terms in
the order the header states (strided lane sums, six butterfly levels, one cast); the values are held to the bounds the unordered
calls are documented with, against the float64 scatters of exits_emulation.py and exits_gradient_emulation.py; and the
dot-product identity ties them to exits_apply / the linear part of exits_apply_gradient.

Scenes, colours, points, frame (16 x 16), depth, shell and intensity are those of tests/test_gpu_exits.py."""
import numpy as np
import pytest

import exits_emulation as xe
import exits_gradient_emulation as xg
import exits_index_emulation as xi
from conftest import box_problem
from test_gpu_exits import BASE, DEPTH, EPS, FRAME, INTENSITY, S, WIDTH, _colors, _make, _points, _same_records, _scene
from test_gpu_parity import _integrator

pytestmark = pytest.mark.gpu

SEED = 70          # the directions' seeds of a list of the gradient; BASE (3000) the walks'
KINDS = ["mixed", "source", "dirichlet", "cube"]
WOST_ERR_INVALID, WOST_ERR_UNSUPPORTED = -1, -3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(_bits(a), _bits(b))


def _walk(it, pts, S_=S, base=BASE):
    stats = it.exits_walk(pts, S_, base, WIDTH)
    assert it.exits_done == (len(pts), S_)
    return it.exits_records(), dict(stats)


def _walk_gradient(it, pts, S_=S):
    stats = it.exits_walk_gradient(pts, S_, SEED, BASE, WIDTH)
    assert it.exits_done == (len(pts), S_)
    return it.exits_records(), it.exits_gradient_records(), dict(stats)


def _lengths(index):
    return np.diff(index["bin_begin"])


def _index(it, rec, prims, n_verts, dim):
    """build the index, hold it to the emulation's integer for integer, return the emulation's"""
    it.exits_index()
    got, want = it.exits_index_records(), xi.build_index(rec, prims, n_verts, dim)
    assert got["bin_begin"].dtype == np.int64 and got["inc"].dtype == np.int32
    assert np.array_equal(got["bin_begin"], want["bin_begin"]) and np.array_equal(got["inc"], want["inc"])
    longest = int(_lengths(want).max())
    assert it.exits_index_info == (len(want["inc"]), longest) and len(want["inc"]) == dim * int((rec["prim"] >= 0).sum())
    return want


# ---- 1. the index, integer for integer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", [1, 8, 65])
@pytest.mark.parametrize("n", [1, 33, 200])
@pytest.mark.parametrize("kind", KINDS)
def test_index_records_equal_the_emulations(kind, n, S_):
    dim, scene, prims, n_verts = _scene(kind)
    it = _make(dim, scene)
    rec, stats = _walk(it, _points(dim)[:n], S_)
    index = _index(it, rec, prims, n_verts, dim)
    it.exits_index()                                                   # a second build is a no-op
    assert np.array_equal(it.exits_index_records()["inc"], index["inc"])
    it.close()
    assert len(index["inc"]) == dim * stats["walks_absorbed"]
    lengths = _lengths(index)
    if n == 1 and S_ == 1:
        assert lengths[lengths > 0].tolist() == [1] * (dim * stats["walks_absorbed"]) and (lengths == 0).any()
    if n == 33 and S_ == 8:
        assert ((lengths > 1) & (lengths < 64)).any()
    if n == 200 and S_ == 65:
        assert lengths.max() > 128                                      # more than two trips of a lane


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_one_absorbed_walk_gives_dim_bins_of_one_entry_and_empty_bins(kind):
    """the point inside the shell is absorbed at depth 0: one walk, dim incidences, each alone in its bin; every other bin -- the
    vertices nobody exits at -- is empty and gets exactly +0.0"""
    dim, scene, prims, n_verts = _scene(kind)
    it = _make(dim, scene)
    rec, stats = _walk(it, _points(dim)[1:2], 1)
    index = _index(it, rec, prims, n_verts, dim)
    v = np.random.default_rng(41).normal(size=(1, 1, 3)).astype(np.float32)
    got = it.exits_adjoint_ordered(v)
    it.close()
    lengths = _lengths(index)
    assert stats["walks_absorbed"] == 1 and lengths[lengths > 0].tolist() == [1] * dim and (lengths == 0).sum() == 2 * n_verts - dim
    assert _same_bits(got, xi.adjoint_ordered(rec, index, v, INTENSITY, dim))
    touched = np.repeat(lengths > 0, 3).reshape(n_verts, 6)[None]
    assert np.all(got[~touched] == 0.0) and not np.signbit(got[~touched]).any() and np.all(got[touched] != 0.0)


def test_bins_of_exactly_64_and_65_entries():
    """a lane's second trip starts at entry 64 of a bin.  One walk per point: a point adds at most one entry to a bin, so the bin
    that ends longest passes through every length on the way, and the list cut where it holds exactly 64, and 65, entries is
    walked and indexed on its own -- a cut list has the same records -- and gathered over, bit for bit.  (Empty bins and bins of
    one entry: the list of one walk in test_index_records_equal_the_emulations; more than 128 entries: its longest list.)"""
    dim, scene, prims, n_verts = _scene("dirichlet")
    pts = np.tile(_points(dim), (16, 1))
    it = _make(dim, scene)
    rec, _ = _walk(it, pts, 1)
    whole = xi.build_index(rec, prims, n_verts, dim)
    b = int(np.argmax(_lengths(whole)))
    assert _lengths(whole)[b] >= 65
    mine = np.sort(whole["inc"][whole["bin_begin"][b]:whole["bin_begin"][b + 1]]) // dim          # the walks (= points) of bin b
    seen = set()
    for want in (64, 65):
        n = int(mine[want - 1]) + 1                                    # the list up to and with the point of entry `want`
        cut, _ = _walk(it, pts[:n], 1)
        assert _same_records(rec, cut, slice(0, n))
        index = _index(it, cut, prims, n_verts, dim)
        lengths = _lengths(index)
        assert lengths[b] == want
        seen |= set(lengths.tolist())
        v = np.random.default_rng(want).normal(size=(2, n, 3)).astype(np.float32)
        assert _same_bits(it.exits_adjoint_ordered(v), xi.adjoint_ordered(cut, index, v, INTENSITY, dim))
    it.close()
    assert {64, 65} <= seen and any(x < 64 for x in seen)


# ---- 2. / 4. the ordered adjoint, bit for bit, and within the bound of the unordered one --------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_adjoint_ordered_equals_the_emulation_bit_for_bit(kind, K):
    """200 points, 8 walks: the point on the boundary and the one in its shell (absorbed at depth 0), the far point, points on
    both sides; and a longer wave's worth at 65 walks for the first 40"""
    dim, scene, prims, n_verts = _scene(kind)
    it = _make(dim, scene)
    for n, S_ in ((200, 8), (40, 65)):
        pts = _points(dim)[:n]
        v = np.random.default_rng(17 + K).normal(size=(K, n, 3)).astype(np.float32)
        rec, _ = _walk(it, pts, S_)
        index = _index(it, rec, prims, n_verts, dim)
        got = it.exits_adjoint_ordered(v)
        plain = it.exits_adjoint(v)
        want = xi.adjoint_ordered(rec, index, v, INTENSITY, dim)
        assert got.shape == (K, n_verts, 6) and _same_bits(got, want), float(np.abs(got - want).max())
        if K == 1:
            assert _same_bits(it.exits_adjoint_ordered(v[0]), want)
        # the value: within the documented bound of the exact sum, as the unordered call is -- and so within two of each other
        emu = xe.adjoint(rec, v, prims, n_verts, INTENSITY, dim)
        bound = xe.adjoint_bound(emu)
        assert np.all(np.abs(got.astype(np.float64) - emu["value"]) <= bound)
        assert np.all(np.abs(plain.astype(np.float64) - emu["value"]) <= bound)      # (the existing call's own criterion, on this list)
        assert np.all(np.abs(got.astype(np.float64) - plain.astype(np.float64)) <= 2.0 * bound)
        empty = emu["terms"] == 0
        assert np.array_equal(empty, np.repeat(_lengths(index) == 0, 3).reshape(n_verts, 6)[None].repeat(K, 0))
        assert np.all(got[empty] == 0.0) and not np.signbit(got[empty]).any()
    it.close()


@pytest.mark.parametrize("S_,K", [(2, 1), (8, 3), (65, 1)])
@pytest.mark.parametrize("kind", KINDS[:1] + KINDS[2:])
def test_adjoint_gradient_ordered_equals_the_emulation_bit_for_bit(kind, S_, K):
    """the first two points are degenerate (on the boundary, inside the shell): their walks are absorbed and indexed, and their
    incidences are skipped -- dgrad holds NaN there, which a read would spread"""
    dim, scene, prims, n_verts = _scene(kind)
    n = 70
    pts = _points(dim)[:n]
    dgrad = np.random.default_rng(23 + S_).normal(size=(K, n, dim, 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, grec, _ = _walk_gradient(it, pts, S_)
    deg = xg.degenerate(grec["radius"], EPS)
    assert deg[0] and deg[1] and not deg[2] and not deg[3] and np.all(rec["prim"][1] >= 0)      # (absorbed, indexed, skipped)
    dgrad[:, deg] = np.nan
    index = _index(it, rec, prims, n_verts, dim)
    got, plain = it.exits_adjoint_gradient_ordered(dgrad), it.exits_adjoint_gradient(dgrad)
    it.close()
    want = xi.adjoint_gradient_ordered(rec, grec, index, dgrad, INTENSITY, EPS, dim)
    assert got.shape == (K, n_verts, 6) and np.all(np.isfinite(got)) and _same_bits(got, want), float(np.abs(got - want).max())
    emu = xg.adjoint(rec, grec, np.nan_to_num(dgrad), prims, n_verts, INTENSITY, EPS, dim)
    bound = xg.adjoint_bound(emu)
    assert np.all(np.abs(got.astype(np.float64) - emu["value"]) <= bound)
    assert np.all(np.abs(plain.astype(np.float64) - emu["value"]) <= bound)
    assert np.all(got[emu["terms"] == 0] == 0.0) and not np.signbit(got[emu["terms"] == 0]).any() and np.any(got != 0.0)


# ---- 3. the same bits on every run, every stream, host and device form; a NaN point --------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_two_calls_two_streams_and_both_forms_give_the_same_bits(kind):
    import torch
    dim, scene, prims, n_verts = _scene(kind)
    n, K = 70, 2
    pts = _points(dim)[:n].copy()
    pts[37, 1] = np.nan                                                # only the _dev walk lets it in: never walked, exits nowhere
    rng = np.random.default_rng(29)
    v, dgrad = rng.normal(size=(K, n, 3)).astype(np.float32), rng.normal(size=(K, n, dim, 3)).astype(np.float32)
    dgrad[:, 37] = np.nan
    it = _make(dim, scene)
    own = torch.cuda.current_stream().cuda_stream
    other = torch.cuda.Stream()
    d_pts, d_v, d_dgrad = torch.from_numpy(pts).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(dgrad).cuda()
    torch.cuda.synchronize()

    def dev(name, d_in, stream):
        out = torch.full((K, n_verts, 6), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        getattr(it, name)(d_in.data_ptr(), K, out.data_ptr(), stream)      # (complete on return)
        return out.cpu().numpy()

    # the plain list
    it.exits_walk_dev(d_pts.data_ptr(), n, S, own, BASE, WIDTH)
    rec = it.exits_records()
    assert np.all(rec["prim"][37] == -1)
    index = _index(it, rec, prims, n_verts, dim)
    want = xi.adjoint_ordered(rec, index, v, INTENSITY, dim)
    results = [it.exits_adjoint_ordered(v), it.exits_adjoint_ordered(v), dev("exits_adjoint_ordered_dev", d_v, own),
               dev("exits_adjoint_ordered_dev", d_v, other.cuda_stream), dev("exits_adjoint_ordered_dev", d_v, None)]
    assert all(_same_bits(r, want) for r in results)
    # the list of the gradient
    it.exits_walk_gradient_dev(d_pts.data_ptr(), n, S, own, SEED, BASE, WIDTH)
    assert it.exits_index_info == (0, 0)
    rec, grec = it.exits_records(), it.exits_gradient_records()
    assert np.isnan(grec["radius"][37]) and np.all(rec["prim"][37] == -1)
    index = _index(it, rec, prims, n_verts, dim)
    want = xi.adjoint_gradient_ordered(rec, grec, index, dgrad, INTENSITY, EPS, dim)
    results = [it.exits_adjoint_gradient_ordered(dgrad), it.exits_adjoint_gradient_ordered(dgrad),
               dev("exits_adjoint_gradient_ordered_dev", d_dgrad, own), dev("exits_adjoint_gradient_ordered_dev", d_dgrad, other.cuda_stream)]
    assert all(_same_bits(r, want) for r in results) and np.all(np.isfinite(want))
    # ... and the plain ordered adjoint works on it as on any list
    assert _same_bits(it.exits_adjoint_ordered(v), xi.adjoint_ordered(rec, index, v, INTENSITY, dim))
    it.close()


# ---- 5. the dot-product identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "source", "cube"])
def test_the_dot_product_identity_with_apply(kind):
    """as tests/test_gpu_exits.py phrases it for the unordered adjoint: on the difference of two sets of colours
    sum (field_A - field_B) v = sum (c_A - c_B) adjoint(v), to within the fp32 roundings of field and adjoint"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    K = 2
    v = np.random.default_rng(17).normal(size=(K, len(pts), 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, _ = _walk(it, pts)
    it.exits_index()
    got = it.exits_adjoint_ordered(v)
    cA, cB = np.stack([_colors(n_verts, 300 + k) for k in range(K)]), np.stack([_colors(n_verts, 400 + k) for k in range(K)])
    fA, fB = it.exits_apply(cA), it.exits_apply(cB)
    it.close()
    eA, eB = xe.apply(rec, cA, prims, INTENSITY, dim), xe.apply(rec, cB, prims, INTENSITY, dim)
    m = sum(np.maximum(np.abs(e["W"]), np.abs(rec["base"])[None]).astype(np.float64).mean(2) for e in (eA, eB))
    v64 = v.astype(np.float64)
    lhs = float(((fA.astype(np.float64) - fB.astype(np.float64)) * v64).sum())
    rhs = float(((cA.astype(np.float64) - cB.astype(np.float64)) * got.astype(np.float64)).sum())
    tol = 2.0 ** -24 * float((np.abs(v64) * (np.abs(fA) + np.abs(fB) + 10.0 * m)).sum() + (np.abs(cA - cB) * np.abs(got)).sum())
    print("identity: lhs %.9g rhs %.9g, |difference| / tolerance %.3f" % (lhs, rhs, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol * (1.0 + 1e-6) and abs(lhs) > 1e3 * tol


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_the_dot_product_identity_with_apply_gradient(kind):
    """as tests/test_gpu_exits_gradient.py phrases it: <dgrad, J c> = <adjoint(dgrad), c> with J c the emulation's float64 linear
    part, within sum |c| (adjoint_bound + identity_slack)"""
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:70]
    K = 2
    dgrad = np.random.default_rng(17).normal(size=(K, len(pts), dim, 3)).astype(np.float32)
    it = _make(dim, scene)
    rec, grec, _ = _walk_gradient(it, pts)
    it.exits_index()
    got = it.exits_adjoint_gradient_ordered(dgrad)
    it.close()
    emu = xg.adjoint(rec, grec, dgrad, prims, n_verts, INTENSITY, EPS, dim)
    bound = xg.adjoint_bound(emu)
    c = np.stack([_colors(n_verts, 300 + k) for k in range(K)]).astype(np.float64)
    lhs = float((dgrad.astype(np.float64) * xg.linear(rec, grec, c, prims, INTENSITY, EPS, dim)).sum())
    rhs = float((got.astype(np.float64) * c).sum())
    tol = float((np.abs(c) * (bound + xg.identity_slack(emu))).sum())
    print("identity: lhs %.9g rhs %.9g, |difference| / tolerance %.3f" % (lhs, rhs, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol and abs(lhs) > 1e3 * tol


# ---- 6. lifetime and refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_the_index_lives_and_dies_with_the_list(kind):
    from elaina_amd import capi
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:10]
    v = np.random.default_rng(31).normal(size=(1, 10, 3)).astype(np.float32)
    dgrad = np.random.default_rng(32).normal(size=(1, 10, dim, 3)).astype(np.float32)
    it = _make(dim, scene)
    assert it.exits_index_info == (0, 0)
    with pytest.raises(capi.WostError, match="no exit list is bound"):
        it.exits_index()
    rec, _ = _walk(it, pts)
    # before exits_index(): refused, the message names it, the output is untouched
    with pytest.raises(capi.WostError, match="wost_exits_index"):
        it.exits_adjoint_ordered(v)
    with pytest.raises(capi.WostError, match="wost_exits_index"):
        it.exits_index_records()
    out = np.full((1, n_verts, 6), -1.0, np.float32)
    assert getattr(it.lib, it._prefix + "exits_adjoint_ordered")(it._handle, capi._fp(v), 1, capi._fp(out)) == WOST_ERR_INVALID and np.all(out == -1.0)
    index = _index(it, rec, prims, n_verts, dim)
    first = it.exits_adjoint_ordered(v)
    assert _same_bits(first, xi.adjoint_ordered(rec, index, v, INTENSITY, dim))
    # the gradient form on a plain list: refused, the message names the walk that binds one with directions
    with pytest.raises(capi.WostError, match="wost_exits_walk_gradient"):
        it.exits_adjoint_gradient_ordered(dgrad)
    # a refused walk keeps the list and the index
    with pytest.raises(capi.WostError, match="walk_seed_base"):
        it.exits_walk(pts[:3], S, -1, WIDTH)
    bad = pts.copy()
    bad[4, 0] = np.inf
    with pytest.raises(capi.WostError, match="point 4 "):
        it.exits_walk(bad, S, BASE, WIDTH)
    assert it.exits_index_info == (len(index["inc"]), int(_lengths(index).max())) and _same_bits(it.exits_adjoint_ordered(v), first)
    # a new walk drops the index
    rec2, _ = _walk(it, pts[:6], 3, BASE + 1)
    assert it.exits_index_info == (0, 0)
    with pytest.raises(capi.WostError, match="wost_exits_index"):
        it.exits_adjoint_ordered(v[:, :6])
    index2 = _index(it, rec2, prims, n_verts, dim)
    assert _same_bits(it.exits_adjoint_ordered(v[:, :6]), xi.adjoint_ordered(rec2, index2, v[:, :6], INTENSITY, dim))
    # ... and so does a walk of the gradient, whose list takes both forms once indexed
    rec3, grec3, _ = _walk_gradient(it, pts)
    assert it.exits_index_info == (0, 0)
    with pytest.raises(capi.WostError, match="wost_exits_index"):
        it.exits_adjoint_gradient_ordered(dgrad)
    index3 = _index(it, rec3, prims, n_verts, dim)
    dgrad[:, xg.degenerate(grec3["radius"], EPS)] = np.nan
    assert _same_bits(it.exits_adjoint_gradient_ordered(dgrad), xi.adjoint_gradient_ordered(rec3, grec3, index3, dgrad, INTENSITY, EPS, dim))
    # releasing the list drops the index
    it.exits_walk(pts[:0], S, BASE, WIDTH)
    assert it.exits_done == (0, 0) and it.exits_index_info == (0, 0)
    out = np.full((1, n_verts, 6), -1.0, np.float32)
    assert getattr(it.lib, it._prefix + "exits_adjoint_ordered")(it._handle, capi._fp(v), 1, capi._fp(out)) == WOST_ERR_INVALID
    assert b"no exit list is bound" in it.lib.wost_last_error() and np.all(out == -1.0)
    it.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_a_list_with_no_absorbed_walk_has_an_empty_index_and_gives_zeros(dim):
    """depth 1 from the middle of the domain: every walk ends by truncation"""
    _, scene, prims, n_verts = _scene("mixed" if dim == 2 else "cube")
    it = _make(dim, scene, depth=1)
    pts = np.full((2, dim), 0.5, np.float32)
    pts[1, 0] = 0.45
    rec, stats = _walk(it, pts)
    assert stats["walks_absorbed"] == 0 and np.all(rec["prim"] == -1)
    index = _index(it, rec, prims, n_verts, dim)
    assert it.exits_index_info == (0, 0) and len(index["inc"]) == 0 and np.all(index["bin_begin"] == 0)
    out = it.exits_adjoint_ordered(np.ones((2, 2, 3), np.float32))
    assert out.shape == (2, n_verts, 6) and np.all(out == 0.0) and not np.signbit(out).any()
    rec, grec, stats = _walk_gradient(it, pts)
    assert stats["walks_absorbed"] == 0
    it.exits_index()
    out = it.exits_adjoint_gradient_ordered(np.ones((1, 2, dim, 3), np.float32))
    assert np.all(out == 0.0) and not np.signbit(out).any()
    it.close()


def test_a_scene_without_a_dirichlet_mesh_has_no_index():
    from elaina_amd import capi
    p = box_problem(d_sides=(), n_sides=(0, 1, 2, 3), flux=lambda x, y, s: 0.5)
    it = _integrator(p, FRAME, FRAME, 1, DEPTH, EPS)
    _walk(it, np.random.default_rng(2).uniform(0.2, 0.8, size=(12, 2)).astype(np.float32))
    assert it.lib.wost_exits_index(it._handle) == WOST_ERR_UNSUPPORTED and b"Dirichlet" in it.lib.wost_last_error()
    assert it.exits_index_info == (0, 0)
    d, out = np.zeros((1, 12, 3), np.float32), np.full(6, -1.0, np.float32)
    assert it.lib.wost_exits_adjoint_ordered(it._handle, capi._fp(d), 1, capi._fp(out)) == WOST_ERR_INVALID
    assert b"wost_exits_index" in it.lib.wost_last_error() and np.all(out == -1.0)
    it.close()


@pytest.mark.parametrize("kind", ["mixed", "cube"])
def test_the_index_and_the_neighbours_leave_one_another_alone(kind):
    dim, scene, prims, n_verts = _scene(kind)
    pts = _points(dim)[:60]
    listed = np.random.default_rng(6).uniform(0.1, 0.9, size=(50, dim)).astype(np.float32)
    v = np.random.default_rng(33).normal(size=(2, len(pts), 3)).astype(np.float32)
    sets = np.stack([_colors(n_verts, 700 + k) for k in range(2)])

    def run(with_index):
        it = _make(dim, scene, spp=8)
        out, mine = [], None
        it.solve()
        out.append(it.solution.copy())
        rec, _ = _walk(it, pts)
        if with_index:
            index = _index(it, rec, prims, n_verts, dim)
            mine = [index, it.exits_adjoint_ordered(v)]
        out.append(it.exits_apply(sets))
        it.exits_adjoint(v)                                            # (the unordered adjoint runs beside; its bits are its own)
        out.append(it.solve_points(listed, 9, 16))
        it.solve_more(3)
        out.append(it.solution.copy())
        it.points_carry(listed, 9, 16)
        out.append(it.points_more(2))
        g = it.solve_gradient_points(listed[:20], 500, 1000, 32)
        out += [g["grad"], g["field"]]
        it.gradient_points_carry(listed[:20], 4, max_rounds=2, seed_base=600, walk_seed_base=2000, seed_width=32)
        out.append(it.gradient_points_more()["grad"])
        it.solve()
        out.append(it.solution.copy())
        if with_index:
            got = it.exits_index_records()
            assert it.exits_done == (len(pts), S) and _same_records(rec, it.exits_records())
            assert np.array_equal(got["bin_begin"], mine[0]["bin_begin"]) and np.array_equal(got["inc"], mine[0]["inc"])
            assert _same_bits(it.exits_adjoint_ordered(v), mine[1])
        out.append(it.exits_apply(sets))
        it.close()
        return out

    plain, indexed = run(False), run(True)
    assert np.any(plain[0] != 0) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, indexed))
