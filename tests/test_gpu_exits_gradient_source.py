"""Exit lists of the gradient on a scene with a source term (the option "exits_grad_source"; include/wost.h "Exit lists of the
gradient", item 4): the walk computes the in-ball term T, seT, U once and keeps it per point, apply joins it to every set.

Every check stands on something outside the code under test.  The reference of the outputs is always a SECOND HANDLE with
"grad_source" 1 and spp = S: wost_solve_gradient_points there has to give the very bits exits_apply_gradient gives here, with
the handle's own colours and with any other (a fresh handle made with them).  The term itself is compared with the numpy
emulation of the in-ball samples (gradient_source_emulation.py), the adjoints with the float64 scatter of
exits_gradient_emulation.py and the stated order of exits_index_emulation.py, and the Poisson problem of
tests/test_gpu_gradient_source.py, whose single call is tied to the analytic gradient there, anchors the whole.

Frame 16 x 16 (n_pixels = 256), the scenes and points of tests/test_gpu_gradient_source.py, the seeds of
tests/test_gpu_exits_gradient.py (directions 70, walks 3000, width 16), depth 32, shell 1e-3.

Bounds, all derived and none measured.  The terms against the emulation: those of tests/test_gpu_gradient_source.py for fp64 sums
in any order -- |T - T'| <= 2^-23 (|T'| + (R / S) sum |a_s|), |U - U'| <= 2^-23 (|U'| + (R^2 / S) sum |wu ms|), seT within the
relative 2 S 2^-23 -- which the unrounded fp64 terms of the list meet with room.  The adjoint: exits_gradient_emulation's
adjoint_bound.  The identity <dgrad, grad(c1) - grad(c2)> = <adjoint(dgrad), c1 - c2>: T cancels in the difference; the left
side carries, per entry, the rounding of each fp32 output (2^-24 |grad|) and the fp32 roundings of each walk's W -- at most 10
operations (3-D: two for the first weight, three products, two sums, intensity, throughput, base), each on a number no larger
than A_s = intensity |thp_s| max|c| + |base_s| up to a factor 1.01 -- weighed by scale |n - nbar| <= 2 scale; the fp64 roundings
of the join are covered by a factor 1 + 2^-20; the right side is within sum |c1 - c2| (adjoint_bound + identity_slack).

Mutation check (run once on scratch copies of the library, not part of the suite; all 30 cases pass on the library as it is).
seT left out of the join in the apply kernel fails 16 cases: test_the_handles_own_colours_give_the_single_call_bit_for_bit (all
but n = 1, whose one point is degenerate), both 3-D cases, test_other_colours_match_fresh_handles_made_with_them (both),
test_the_single_call_and_the_carried_list_between_walk_and_apply_change_nothing (both) and the Poisson anchor.  U left out of the
join fails those and test_the_terms_match_the_emulation_of_the_in_ball_samples (both): 18.  U added for degenerate points in the
apply kernel fails NONE, and no test of the library can make it: the walk stores +0.0 for such a point, so that mutant differs
from the library only where a mean is -0.0; what keeps a degenerate point's field free of U is therefore pinned twice over, by
the zeros of the terms (every case of the first two tests and the NaN point of the device forms) and, for the join itself, by
tests/test_exits_gradient_source_cpu.py on terms that are not zero there.  The guard of the walk's side -- the terms kernel storing
what it computes for a degenerate point too -- fails the two cases of
test_device_arrays_on_the_callers_stream_and_a_point_that_is_not_finite (the NaN point's terms are NaN then) and no other: a
degenerate point with a finite radius took no samples, and R times a sum of zeros is zero."""
import ctypes as C

import numpy as np
import pytest

import exits_gradient_emulation as xg
import exits_index_emulation as xi
import gradient_source_emulation as gs
from test_gpu_exits import BASE, WIDTH, _colors, _same_records
from test_gpu_exits_gradient import ALL, SEED
from test_gpu_gradient import BOX, _box_points, _mixed_cube
from test_gpu_gradient_source import POISSON, _cube_points, _poisson, _source_box, _source_cube
from test_gpu_parity import _integrator
from test_gpu_points import COUNTERS, _it3, _mixed_box

pytestmark = pytest.mark.gpu

S, DEPTH, EPS, FRAME = BOX["S"], BOX["depth"], BOX["eps"], 16
WOST_ERR_INVALID, WOST_ERR_UNSUPPORTED = -1, -3
OUT = ("grad", "stderr", "field")
_REF = {}


def _scene(dim, source=True, colors=None):
    if dim == 2:
        p = _source_box() if source else _mixed_box()
        if colors is not None:
            p.d_colors = np.ascontiguousarray(colors, np.float32)
        return p
    sd = _source_cube() if source else _mixed_cube()
    if colors is not None:
        sd["d_colors"] = np.ascontiguousarray(colors, np.float32)
    return sd


def _handle(dim, scene, spp=1, frame=FRAME, depth=DEPTH, eps=EPS, **options):
    it = _integrator(scene, frame, frame, spp, depth, eps) if dim == 2 else _it3(scene, frame, frame, spp, depth, eps)
    for k, v in options.items():
        it.set_option(k, v)
    return it


def _list_handle(dim, source=True, spp=1, **kw):
    """a handle whose walks of the gradient's exit list take a scene with a source term; its spp is not read by the list"""
    return _handle(dim, _scene(dim, source), spp=spp, exits_grad_source=1, **kw)


def _points(dim):
    return _box_points() if dim == 2 else _cube_points()


def _prims(it):
    return it.problem.d_segs if it._dim == 2 else it.problem.d_tris


def _walk(it, pts, S_=S, seed=SEED, base=BASE, width=WIDTH):
    stats = dict(it.exits_walk_gradient(pts, S_, seed, base, width))
    assert it.exits_done == (len(pts), S_)
    return it.exits_records(), it.exits_gradient_records(), stats


def _single(dim, pts, S_=S, colors=None, seed=SEED, base=BASE, key=None):
    """the reference: wost_solve_gradient_points on a second handle with "grad_source" 1 and spp = S_, once per key.  The single
    call refuses S > n_pixels, so past 256 the reference handle has a 32 x 32 frame: its outputs do not depend on the frame"""
    if key is not None and key in _REF:
        return _REF[key]
    ref = _handle(dim, _scene(dim, True, colors), spp=S_, frame=FRAME if S_ <= FRAME * FRAME else 32, grad_source=1)
    out = ref.solve_gradient_points(pts, seed, base, WIDTH, want=ALL, spp=S_)
    stats = dict(ref.last_stats)
    ref.close()
    if key is not None:
        _REF[key] = (out, stats)
    return out, stats


def _same_outputs(got, k, want):
    """set k of exits_apply_gradient against a single call's outputs, bit for bit"""
    return all(np.array_equal(got[a][k], want[a], equal_nan=True) for a in OUT)


def _same_sets(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in OUT)


def _launches(n, S_):
    per_block = max(1, FRAME * FRAME // S_)
    return -(-n // (FRAME * FRAME)) + 2 * -(-n // per_block) + -(-n * S_ // (FRAME * FRAME))


def _assert_the_single_call(dim, n, S_):
    pts = _points(dim)[:n]
    it = _list_handle(dim)
    rec, grec, stats = _walk(it, pts, S_)
    own = it.problem.d_colors
    got = it.exits_apply_gradient(own)
    only = it.exits_apply_gradient(own, want=())
    T, seT, U = it.exits_gradient_terms()
    it.close()
    want, want_stats = _single(dim, pts, S_, key=(dim, n, S_))
    assert got["grad"].shape == (1, n, dim, 3) and got["field"].shape == (1, n, 3) and set(only) == {"grad"}
    assert np.array_equal(grec["radius"], want["radius"]) and np.array_equal(grec["first_pts"], want["first_pts"])
    worst = [float(np.nan_to_num(np.abs(got[a][0].astype(np.float64) - want[a])).max()) for a in OUT]
    print("dim %d n %d S %d: largest |difference| of grad, stderr, field %s" % (dim, n, S_, worst))
    assert _same_outputs(got, 0, want), worst
    assert np.array_equal(only["grad"], got["grad"], equal_nan=True)
    for c in COUNTERS:
        assert stats[c] == want_stats[c], (c, stats[c], want_stats[c])
    assert stats["walks_started"] == n * S_ and stats["kernel_launches"] == _launches(n, S_), (stats["kernel_launches"], _launches(n, S_))
    deg = xg.degenerate(grec["radius"], EPS)
    assert np.all(np.isnan(got["grad"][0][deg])) and np.all(np.isnan(got["stderr"][0][deg])) and np.all(np.isfinite(got["field"]))
    assert np.all(np.isfinite(got["grad"][0][~deg])) and np.all(np.isfinite(got["stderr"][0][~deg]))
    assert T.shape == seT.shape == (n, dim, 3) and U.shape == (n, 3) and T.dtype == seT.dtype == U.dtype == np.float64
    assert not np.any(T[deg]) and not np.any(seT[deg]) and not np.any(U[deg]) and not np.any(np.signbit(U[deg]))
    return deg, got, (T, seT, U)


# ---- 1. bit for bit against the single call, 2-D ---------------------------------------------------------------------------------
CASES2 = [(n, 8) for n in (1, 31, 32, 33, 200)] + [(7, s) for s in (2, 64, 65, 130, 300)]


@pytest.mark.parametrize("n,S_", CASES2)
def test_the_handles_own_colours_give_the_single_call_bit_for_bit(n, S_):
    """S = 8: blocks of 32 points -- a part of one, one short, a block, one more, seven.  n = 7: S = 2, a full wave, 65 (blocks of
    3, the lanes take two trips), 130 and 300 (blocks of one point; at 300 the temporary is sized by S, not by the frame).  The
    first two points are degenerate: NaN, NaN and a finite mean, the reference's"""
    deg, got, (T, seT, U) = _assert_the_single_call(2, n, S_)
    if n >= 4:
        assert deg[0] and deg[1] and not deg[2] and not deg[3]
    if n >= 7:
        assert np.any(T[~deg] != 0) and np.any(seT[~deg] != 0) and np.any(U[~deg] != 0)


# ---- 2. 3-D --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S_", [(100, 8), (5, 65)])
def test_3d_the_handles_own_colours_give_the_single_call_bit_for_bit(n, S_):
    """100 points in blocks of 32, 32, 32 and 4; 5 points of 65 walks in blocks of 3 and 2"""
    deg, got, (T, seT, U) = _assert_the_single_call(3, n, S_)
    assert not deg.any() and np.any(T != 0) and np.any(U != 0)


# ---- 3. other colours ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_other_colours_match_fresh_handles_made_with_them(dim):
    pts = _points(dim)[:70]
    it = _list_handle(dim)
    n_verts = len(it.problem.d_verts)
    sets = np.stack([_colors(n_verts, 200 + k) for k in range(3)])
    _walk(it, pts)
    got = it.exits_apply_gradient(sets)
    ones = [it.exits_apply_gradient(sets[k]) for k in range(3)]
    it.close()
    assert got["grad"].shape == got["stderr"].shape == (3, 70, dim, 3) and got["field"].shape == (3, 70, 3)
    for k in range(3):
        want, _ = _single(dim, pts, colors=sets[k])
        assert _same_outputs(got, k, want), (k, float(np.nanmax(np.abs(got["grad"][k] - want["grad"]))))
        assert all(np.array_equal(ones[k][a][0], got[a][k], equal_nan=True) for a in OUT)
    assert np.any(got["grad"][0] != got["grad"][1])


# ---- 4. the term is there --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_terms_match_the_emulation_of_the_in_ball_samples(oracle, dim):
    n = 33 if dim == 2 else 100
    pts = _points(dim)[:n]
    it = _list_handle(dim)
    sd = it.problem.as_dict() if dim == 2 else _source_cube()
    rec, grec, _ = _walk(it, pts)
    T, seT, U = it.exits_gradient_terms()
    assert getattr(it.lib, it._prefix + "exits_gradient_terms")(it._handle, None, None, None) == 0      # "does the list carry the term": yes
    sets = np.stack([it.problem.d_colors, _colors(len(it.problem.d_verts), 210)])
    both = it.exits_apply_gradient(sets)
    field = it.exits_apply(sets)
    # ... and exits_apply on it is the mean of the walks from the first points: a plain list of them, one walk each
    it.exits_walk(grec["first_pts"].reshape(-1, dim), 1, BASE, WIDTH)
    plain_rec, W = it.exits_records(), it.exits_apply(sets).reshape(2, n, S, 3).astype(np.float64)
    it.close()
    deg = xg.degenerate(grec["radius"], EPS)
    smp = gs.samples(oracle, "box-source" if dim == 2 else "cube-source", sd, pts, grec["radius"], deg, S, SEED, WIDTH, dim)
    red = gs.reduce(smp, grec["radius"])
    ok = ~deg
    tol_T, tol_U = 2.0 ** -23 * (np.abs(red["T"]) + red["mag_T"]), 2.0 ** -23 * (np.abs(red["U"]) + red["mag_U"])
    assert ok.sum() >= n - 3
    assert np.all(np.abs(T[ok] - red["T"][ok]) <= tol_T[ok]) and np.all(np.abs(U[ok] - red["U"][ok]) <= tol_U[ok])
    assert np.all(np.abs(seT[ok] - red["seT"][ok]) <= 2.0 * S * 2.0 ** -23 * red["seT"][ok])
    print("dim %d: max |T - T'| / tol %.3g, |U - U'| / tol %.3g" % (dim, float((np.abs(T - red["T"])[ok] / np.maximum(tol_T[ok], 1e-300)).max()),
                                                                   float((np.abs(U - red["U"])[ok] / np.maximum(tol_U[ok], 1e-300)).max())))
    # the term is no rounding error
    assert np.any(np.abs(T[ok]) > 10.0 * tol_T[ok]) and np.any(np.abs(U[ok]) > 10.0 * tol_U[ok])
    assert not np.any(T[deg]) and not np.any(seT[deg]) and not np.any(U[deg])
    # the field of exits_apply carries no U: it is the fp64 mean of the plain list's fp32 W, rounded once (any order of the sum)
    assert all(np.array_equal(rec[k].reshape(plain_rec[k].shape), plain_rec[k], equal_nan=True) for k in rec)
    mean = W.sum(axis=2) / S
    bound = 2.0 ** -24 * np.abs(mean) + S * 2.0 ** -53 * np.abs(W).sum(axis=2)
    assert np.all(np.abs(field.astype(np.float64) - mean) <= bound)
    # (two fp32 roundings of numbers that differ by U: 2^-24 of each, relative to the rounded value at most 2^-23)
    with_u = both["field"].astype(np.float64) - field
    assert np.all(np.abs(with_u[:, ok] - U[None, ok]) <= 2.0 ** -23 * (np.abs(both["field"][:, ok]) + np.abs(field[:, ok])))
    assert np.any(np.abs(U[ok]) > 10.0 * bound[0][ok]) and np.array_equal(both["field"][:, deg], field[:, deg])


# ---- 5. the adjoints on a source scene ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_adjoints_on_a_source_scene(dim):
    pts = _points(dim)[:70]
    n = len(pts)
    it = _list_handle(dim)
    prims, n_verts, intensity = _prims(it), len(it.problem.d_verts), it.problem.dirichlet_intensity
    dgrad = np.random.default_rng(17).normal(size=(1, n, dim, 3)).astype(np.float32)
    v = np.random.default_rng(18).normal(size=(1, n, 3)).astype(np.float32)
    sets = np.stack([_colors(n_verts, 300 + k) for k in range(2)])
    rec, grec, _ = _walk(it, pts)
    adj = it.exits_adjoint_gradient(dgrad)
    out = it.exits_apply_gradient(sets, want=())
    it.exits_index()
    ordered = it.exits_adjoint_ordered(v), it.exits_adjoint_gradient_ordered(dgrad)
    it.set_option("exits_grad_source", 0)          # the adjoints read the list, not the option
    adj_off = it.exits_adjoint_gradient(dgrad)
    ordered_off = it.exits_adjoint_ordered(v), it.exits_adjoint_gradient_ordered(dgrad)
    it.close()
    emu = xg.adjoint(rec, grec, dgrad, prims, n_verts, intensity, EPS, dim)
    bound = xg.adjoint_bound(emu)
    for a in (adj, adj_off):
        err = np.abs(a.astype(np.float64) - emu["value"])
        assert a.shape == (1, n_verts, 6) and np.all(err <= bound), float((err - bound).max())
        assert np.all(a[emu["terms"] == 0] == 0.0)
    deg = xg.degenerate(grec["radius"], EPS)
    assert np.any(emu["terms"] > 1) and (dim == 3 or deg.any())
    # the identity on the linear part: T cancels in grad(c1) - grad(c2)
    ok = ~deg
    g1, g2 = out["grad"][0][ok].astype(np.float64), out["grad"][1][ok].astype(np.float64)
    d64, dc = dgrad[0][ok].astype(np.float64), sets[0].astype(np.float64) - sets[1].astype(np.float64)
    lhs, rhs = float((d64 * (g1 - g2)).sum()), float((adj[0].astype(np.float64) * dc).sum())
    scale = dim / (grec["radius"][ok].astype(np.float64) * (S - 1))
    A = sum(float(intensity) * np.abs(rec["thp"][ok].astype(np.float64))[:, :, None] * float(np.abs(c).max()) + np.abs(rec["base"][ok].astype(np.float64))
            for c in sets).sum(axis=1)                                                             # (n, 3): both sets, all walks
    per_entry = 2.0 ** -24 * (np.abs(g1) + np.abs(g2)) + (2.0 * scale[:, None] * 10.0 * 2.0 ** -24 * 1.01 * A)[:, None, :]
    tol = (1.0 + 2.0 ** -20) * float((np.abs(d64) * per_entry).sum()) + float((np.abs(dc) * (bound[0] + xg.identity_slack(emu)[0])).sum())
    print("dim %d identity: lhs %.9g rhs %.9g, |difference| / tolerance %.3f" % (dim, lhs, rhs, abs(lhs - rhs) / tol))
    assert abs(lhs - rhs) <= tol and abs(lhs) > 10.0 * tol
    # the ordered adjoints: the stated order, bit for bit, whatever the option says afterwards
    index = xi.build_index(rec, prims, n_verts, dim)
    want = xi.adjoint_ordered(rec, index, v, intensity, dim), xi.adjoint_gradient_ordered(rec, grec, index, dgrad, intensity, EPS, dim)
    for got in (ordered, ordered_off):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.any(want[0] != 0) and np.any(want[1] != 0)


# ---- 6. the mode is the list's -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_mode_is_recorded_in_the_list_at_the_walk(dim):
    from elaina_amd import capi
    pts = _points(dim)[:40]
    it = _list_handle(dim)
    own = it.problem.d_colors
    rec, grec, _ = _walk(it, pts)
    before, terms = it.exits_apply_gradient(own), it.exits_gradient_terms()
    it.set_option("exits_grad_source", 0)
    assert _same_sets(before, it.exits_apply_gradient(own))
    # a second walk is refused now, and says which option opens the door; the list and its outputs stand
    st = capi.Stats()
    fn = getattr(it.lib, it._prefix + "exits_walk_gradient")
    rc = fn(it._handle, capi._fp(pts[:10]), 10, S, SEED, BASE, WIDTH, C.byref(st))
    msg = it.lib.wost_last_error()
    assert rc == WOST_ERR_UNSUPPORTED and b"source term" in msg and b"exits_grad_source" in msg, msg
    assert it.exits_done == (len(pts), S) and _same_records(rec, it.exits_records())
    assert all(np.array_equal(grec[k], w, equal_nan=True) for k, w in it.exits_gradient_records().items())
    assert _same_sets(before, it.exits_apply_gradient(own)) and all(np.array_equal(a, b) for a, b in zip(terms, it.exits_gradient_terms()))
    # "grad_source" is another key: it does not open this door
    it.set_option("grad_source", 1)
    assert fn(it._handle, capi._fp(pts[:10]), 10, S, SEED, BASE, WIDTH, C.byref(st)) == WOST_ERR_UNSUPPORTED
    it.set_option("exits_grad_source", 1)
    _walk(it, pts[:10])
    assert it.exits_done == (10, S) and _same_sets({k: before[k][:, :10] for k in OUT}, it.exits_apply_gradient(own))
    it.close()


# ---- 7. the cut ------------------------------------------------------------------------------------------------------------------------
def test_a_cut_list_gives_the_same_rows_and_terms():
    pts = _points(2)
    it = _list_handle(2)
    sets = np.stack([_colors(len(it.problem.d_verts), 500 + k) for k in range(2)])
    rec, grec, _ = _walk(it, pts)
    whole, terms = it.exits_apply_gradient(sets), it.exits_gradient_terms()
    hrec, hgrec, _ = _walk(it, pts[:77])
    head, hterms = it.exits_apply_gradient(sets), it.exits_gradient_terms()
    trec, tgrec, _ = _walk(it, pts[77:], seed=SEED + 77, base=BASE + 77 * S)
    tail, tterms = it.exits_apply_gradient(sets), it.exits_gradient_terms()
    it.close()
    assert _same_records(rec, hrec, slice(0, 77)) and _same_records(rec, trec, slice(77, None))
    for k in grec:
        assert np.array_equal(grec[k][:77], hgrec[k]) and np.array_equal(grec[k][77:], tgrec[k])
    for k in OUT:
        assert np.array_equal(whole[k][:, :77], head[k], equal_nan=True) and np.array_equal(whole[k][:, 77:], tail[k], equal_nan=True)
    for a, h, t in zip(terms, hterms, tterms):
        assert np.array_equal(a[:77], h) and np.array_equal(a[77:], t) and np.any(a != 0)


# ---- 8. device forms and a NaN point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_device_arrays_on_the_callers_stream_and_a_point_that_is_not_finite(dim):
    import torch
    pts = _points(dim)[:70]
    n, K = len(pts), 2
    it = _list_handle(dim)
    n_verts = len(it.problem.d_verts)
    sets = np.stack([_colors(n_verts, 600 + k) for k in range(K)])
    host_rec, host_grec, host_stats = _walk(it, pts)
    host, host_terms = it.exits_apply_gradient(sets), it.exits_gradient_terms()
    stream = torch.cuda.current_stream().cuda_stream

    def on_device(p):
        d_pts = torch.from_numpy(p).cuda()
        stats = dict(it.exits_walk_gradient_dev(d_pts.data_ptr(), n, S, stream, SEED, BASE, WIDTH))
        d_sets = torch.from_numpy(sets).cuda()
        grad, se = (torch.full((K, n, dim, 3), -1.0, dtype=torch.float32, device="cuda") for _ in range(2))
        field = torch.full((K, n, 3), -1.0, dtype=torch.float32, device="cuda")
        it.exits_apply_gradient_dev(d_sets.data_ptr(), K, grad.data_ptr(), stream, se.data_ptr(), field.data_ptr())
        return it.exits_records(), stats, {"grad": grad.cpu().numpy(), "stderr": se.cpu().numpy(), "field": field.cpu().numpy()}, it.exits_gradient_terms()

    rec, stats, out, terms = on_device(pts)
    assert _same_records(host_rec, rec) and _same_sets(host, out) and all(np.array_equal(a, b) for a, b in zip(host_terms, terms))
    for c in COUNTERS + ("kernel_launches",):
        assert stats[c] == host_stats[c], c
    # a NaN coordinate: that point is never walked and takes no samples -- NaN outputs, zero terms; its neighbours keep their bits
    bad = pts.copy()
    bad[37, 1] = np.nan
    rec, stats, out, terms = on_device(bad)
    it.close()
    rest = np.arange(n) != 37
    assert np.all(rec["prim"][37] == -1) and np.all(np.isnan(rec["thp"][37]))
    assert all(np.all(np.isnan(out[k][:, 37])) and np.array_equal(out[k][:, rest], host[k][:, rest], equal_nan=True) for k in OUT)
    assert all(not np.any(a[37]) and not np.any(np.signbit(a[37])) and np.array_equal(a[rest], b[rest]) for a, b in zip(terms, host_terms))
    assert stats["walks_started"] == (n - 1) * S


# ---- 9. neighbours ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_single_call_and_the_carried_list_between_walk_and_apply_change_nothing(dim):
    """the in-ball samples of the walk pass through a temporary of its own, not through the scratch the gradient calls share"""
    pts = _points(dim)[:60]
    other = _points(dim)[60:100]

    def neighbours(it):
        g = it.solve_gradient_points(other, 500, 1000, 32, want=ALL)
        it.gradient_points_carry(other[:20], 4, max_rounds=2, seed_base=600, walk_seed_base=2000, seed_width=32)
        c = it.gradient_points_more()
        return [g[k] for k in sorted(g)] + [c[k] for k in sorted(c)]

    alone = _list_handle(dim, spp=S, grad_source=1)
    want_neighbours = neighbours(alone)
    alone.close()
    it = _list_handle(dim, spp=S, grad_source=1)
    own = it.problem.d_colors
    rec, grec, _ = _walk(it, pts)
    terms = it.exits_gradient_terms()
    got_neighbours = neighbours(it)
    after = it.exits_apply_gradient(own)
    assert _same_records(rec, it.exits_records()) and all(np.array_equal(a, b) for a, b in zip(terms, it.exits_gradient_terms()))
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want_neighbours, got_neighbours))
    # ... and the other way round: a walk behind them
    _walk(it, pts)
    again = it.exits_apply_gradient(own)
    it.close()
    want, _ = _single(dim, pts, key=(dim, "neighbours"))
    assert _same_outputs(after, 0, want) and _same_sets(after, again)


# ---- 10. no source term ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_the_option_changes_nothing_on_a_scene_without_a_source_term(dim):
    from elaina_amd import capi
    pts = _points(dim)[:70]
    runs = []
    for option in (0, 1):
        it = _handle(dim, _scene(dim, source=False), exits_grad_source=option)
        rec, grec, stats = _walk(it, pts)
        runs.append((rec, grec, stats, it.exits_apply_gradient(it.problem.d_colors)))
        for call in (it.exits_gradient_terms, lambda: _check_question(it)):
            with pytest.raises(capi.WostError, match=r"\(-1\).*exits_grad_source"):
                call()
        it.close()
    (rec0, grec0, stats0, out0), (rec1, grec1, stats1, out1) = runs
    assert _same_records(rec0, rec1) and all(np.array_equal(grec0[k], grec1[k]) for k in grec0) and _same_sets(out0, out1)
    for c in COUNTERS + ("kernel_launches",):
        assert stats0[c] == stats1[c], c
    assert stats1["kernel_launches"] == 1 + -(-len(pts) * S // (FRAME * FRAME)) and np.any(np.isfinite(out0["grad"]))


def _check_question(it):
    """the reader with three null pointers: does the bound list carry the term"""
    from elaina_amd.capi import _check
    _check(getattr(it.lib, it._prefix + "exits_gradient_terms")(it._handle, None, None, None), it._prefix + "exits_gradient_terms")


# ---- 11. refusals with the handle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_refusals_that_need_the_handle(dim):
    from elaina_amd import capi
    pts = _points(dim)[:10]
    it = _list_handle(dim)
    for call in (it.exits_gradient_terms, lambda: _check_question(it)):
        with pytest.raises(capi.WostError, match=r"\(-1\).*no exit list is bound"):
            call()
    it.exits_walk(pts, S, BASE, WIDTH)
    for call in (it.exits_gradient_terms, lambda: _check_question(it)):
        with pytest.raises(capi.WostError, match=r"\(-1\).*wost_exits_walk_gradient"):
            call()
    for bad in (0.5, 2, -1, float("nan")):
        with pytest.raises(capi.WostError, match=r"\(-1\).*exits_grad_source"):
            it.set_option("exits_grad_source", bad)
    _walk(it, pts)                                   # (the refused values left the option at 1)
    _check_question(it)
    it.close()


# ---- 12. the analytic anchor -------------------------------------------------------------------------------------------------------------
def test_the_poisson_problem_gives_the_single_calls_bits():
    """the 2-D Poisson problem of tests/test_gpu_gradient_source.py at its own S = 1024 and seeds: that single call is tied to the
    analytic gradient there (the statistical criterion is not run a second time), and the list has to give its bits"""
    ref, pts = _poisson(2)
    ref.set_option("grad_source", 1)
    want = ref.solve_gradient_points(pts, POISSON["seed_base"], POISSON["walk_seed_base"], POISSON["seed_width"], want=ALL, spp=POISSON["S"])
    ref.close()
    it, _ = _poisson(2)
    it.set_option("exits_grad_source", 1)
    stats = it.exits_walk_gradient(pts, POISSON["S"], POISSON["seed_base"], POISSON["walk_seed_base"], POISSON["seed_width"])
    got = it.exits_apply_gradient(it.problem.d_colors)
    T, seT, U = it.exits_gradient_terms()
    it.close()
    assert stats["walks_started"] == len(pts) * POISSON["S"] and _same_outputs(got, 0, want)
    assert np.all(np.isfinite(got["grad"])) and np.all(got["stderr"] > 0)
    # channel 0 has the slope b = 6 along x: T_x = b R^2 / 8 there, within 5 of its own standard error
    R = want["radius"].astype(np.float64)
    assert np.all(np.abs(T[:, 0, 0] - POISSON["ab"][0][1] * R * R / 8.0) <= 5.0 * seT[:, 0, 0])
