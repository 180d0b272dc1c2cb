"""The estimator of wost_solve_gradient_points (include/wost.h) in numpy on top of the oracle.  No tests here:
test_gpu_gradient.py compares the library against it.

The oracle has no gradient, but it has everything the estimator is made of: the closest-point distances (the radius), the PCG32
stream and sincos_2pi (the directions), and -- through the identity of test_gpu_points._oracle_points, a probe of scale 0 at p
walks p on the stream of the solved pixel -- the walk from a first point.  The first points are taken AS GIVEN (the library's
own first_pts), so a last-bit difference in y cannot send a walk elsewhere; they are checked on their own, to one ulp."""
import ctypes as C

import numpy as np

from oracle.oracle import Settings as _Settings, Stats as _Stats, _fp

COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits")
NEUMANN_SHRINK = np.float32(0.875)
_WALKS, _DIRS = {}, {}


def radius(oracle, sd, pts, dim):
    """(R, dD, dN) in float32: R = min(dD, 0.875f * dN) of the oracle's distances, +inf for a mesh the scene does not have"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, dim)
    prims = "segs" if dim == 2 else "tris"

    def dist(which):
        verts, p = sd.get(which + "_verts"), sd.get(which + "_" + prims)
        if verts is None or p is None or len(p) == 0:
            return np.full(len(pts), np.inf, np.float32)
        return (oracle.closest_point(verts, p, pts) if dim == 2 else oracle.closest_point3(verts, p, pts))[1]

    dD, dN = dist("d"), dist("n")
    return np.minimum(dD, NEUMANN_SHRINK * dN).astype(np.float32), dD, dN


def directions(oracle, n, S, seed_base, seed_width, dim):
    """(n, S, dim) float32: S consecutive draws from the stream of pixel seed_base + i, in the library's float32 operations"""
    key = (n, S, seed_base, seed_width, dim)
    if key not in _DIRS:
        one, two = np.float32(1), np.float32(2)
        out = np.zeros((n, S, dim), np.float32)
        for i in range(n):
            r = oracle.pcg_seed_pixel(seed_base + i, seed_width)
            for s in range(S):
                if dim == 2:
                    out[i, s] = oracle.sincos_2pi(oracle.pcg_float(r))
                else:
                    u1, u2 = np.float32(oracle.pcg_float(r)), oracle.pcg_float(r)
                    c, sn = oracle.sincos_2pi(u2)
                    z = one - two * u1
                    rr = np.sqrt(one - z * z)
                    out[i, s] = (rr * np.float32(c), rr * np.float32(sn), z)
        _DIRS[key] = out
    return _DIRS[key]


def walks(oracle, key, sd, first_pts, walk_seed_base, seed_width, depth, eps, dim):
    """W (n, S, 3) float32 and the five counters summed over the walks: walk (i, s) is one oracle solve of one sample of pixel
    walk_seed_base + i * S + s with a zero-scale probe at first_pts[i, s].  A walk is solved once per (key, pixel, first point)."""
    n, S = first_pts.shape[:2]
    height = -(-(walk_seed_base + n * S) // seed_width)
    sc = (oracle.make_scene if dim == 2 else oracle.make_scene3)(dict(sd))
    keep = list(oracle._keep)      # the scene points into these arrays; the oracle's next batch query lets go of them
    sc.probe_scale = 0.0
    if dim == 2:
        sc.probe_up[0], sc.probe_up[1] = 0.0, 1.0
    else:
        for k, (u, r) in enumerate(zip((0.0, 1.0, 0.0), (1.0, 0.0, 0.0))):
            sc.probe_up[k], sc.probe_right[k] = u, r
    st = _Settings(seed_width, height, 1, depth, eps)
    field, stats = np.zeros((1, 3), np.float32), _Stats()
    W = np.zeros((n, S, 3), np.float32)
    total = dict.fromkeys(COUNTERS, 0)
    for i in range(n):
        for s in range(S):
            k, y = walk_seed_base + i * S + s, first_pts[i, s]
            ck = (key, k, seed_width, y.tobytes())
            if ck not in _WALKS:
                for a in range(dim):
                    sc.probe_pos[a] = float(y[a])
                if dim == 2:
                    rc = oracle.lib.wo_solve(C.byref(sc), C.byref(st), k, k + 1, 1, _fp(field), None, None, C.byref(stats))
                else:
                    rc = oracle.lib.wo3_solve(C.byref(sc), C.byref(st), k, k + 1, 1, _fp(field), C.byref(stats))
                assert rc == 0
                _WALKS[ck] = (field[0].copy(), tuple(int(getattr(stats, c)) for c in COUNTERS))
            W[i, s] = _WALKS[ck][0]
            for c, v in zip(COUNTERS, _WALKS[ck][1]):
                total[c] += v
    del keep
    return W, total


def estimate(W, dirs, R, eps, dim):
    """the reduction in float64 from the float32 W, directions and radii, with the bounds of the issue for fp32 sums in any order:
    grad within S 2^-23 d / (R (S - 1)) sum_s |n_sk| (|W_s| + |mean|), field within S 2^-24 mean_s |W_s|"""
    S = W.shape[1]
    W64, n64, R64 = W.astype(np.float64), dirs.astype(np.float64), R.astype(np.float64)[:, None, None]
    mean = W64.mean(axis=1)
    t = n64[:, :, :, None] * (W64 - mean[:, None, :])[:, :, None, :]          # (n, S, dim, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = dim / (R64 * (S - 1)) * t.sum(axis=1)
        se = dim / R64 * np.sqrt(((t - t.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (S - 1) / S)
        mag = (np.abs(n64)[:, :, :, None] * (np.abs(W64) + np.abs(mean)[:, None, :])[:, :, None, :]).sum(axis=1)
        tol_grad = S * 2.0 ** -23 * dim / (R64 * (S - 1)) * mag
    degenerate = ~(R > np.float32(eps)) | ~np.isfinite(R)
    grad[degenerate] = se[degenerate] = np.nan
    return {"grad": grad, "stderr": se, "field": mean, "tol_grad": tol_grad, "tol_field": S * 2.0 ** -24 * np.abs(W64).mean(axis=1),
            "degenerate": degenerate}


def emulate(oracle, key, sd, pts, first_pts, seed_base, walk_seed_base, seed_width, depth, eps, dim):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, dim)
    first_pts = np.ascontiguousarray(first_pts, np.float32).reshape(len(pts), -1, dim)
    R, dD, dN = radius(oracle, sd, pts, dim)
    dirs = directions(oracle, len(pts), first_pts.shape[1], seed_base, seed_width, dim)
    W, counters = walks(oracle, key, sd, first_pts, walk_seed_base, seed_width, depth, eps, dim)
    out = {"R": R, "dD": dD, "dN": dN, "dirs": dirs, "W": W, "counters": counters}
    out.update(estimate(W, dirs, R, eps, dim))
    return out


def assert_first_points(pts, first_pts, emu):
    """y = x + R n to 1 ulp of max(|x_k|, R) (the library fuses the product into the sum); a degenerate point walks from itself"""
    x = np.ascontiguousarray(pts, np.float32).reshape(len(emu["R"]), 1, -1)
    deg = emu["degenerate"]
    assert np.array_equal(first_pts[deg], np.broadcast_to(x, first_pts.shape)[deg])
    ok = ~deg
    want = x[ok].astype(np.float64) + emu["R"][ok].astype(np.float64)[:, None, None] * emu["dirs"][ok].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(x[ok]), emu["R"][ok][:, None, None]).astype(np.float32)).astype(np.float64)
    err = np.abs(first_pts[ok].astype(np.float64) - want)
    assert np.all(err <= ulp), float((err / ulp).max())


def assert_matches(out, stats, emu, pts):
    """every output of a gradient call (a dict with all of grad, stderr, field, radius, first_pts) and its counters against the
    emulation of its own first points"""
    S = out["first_pts"].shape[1]
    assert np.array_equal(out["radius"], emu["R"]), (out["radius"], emu["R"])
    assert_first_points(pts, out["first_pts"], emu)
    for c in COUNTERS:
        assert stats[c] == emu["counters"][c], (c, stats[c], emu["counters"][c])
    deg, ok = emu["degenerate"], ~emu["degenerate"]
    assert np.all(np.isnan(out["grad"][deg])) and np.all(np.isnan(out["stderr"][deg]))
    err = np.abs(out["grad"][ok].astype(np.float64) - emu["grad"][ok])
    assert np.all(err <= emu["tol_grad"][ok]), float((err / np.maximum(emu["tol_grad"][ok], 1e-300)).max())
    err = np.abs(out["field"].astype(np.float64) - emu["field"])
    assert np.all(err <= emu["tol_field"]), float((err / np.maximum(emu["tol_field"], 1e-300)).max())
    err = np.abs(out["stderr"][ok].astype(np.float64) - emu["stderr"][ok])
    assert np.all(err <= 2 * S * 2.0 ** -23 * emu["stderr"][ok]), float((err / np.maximum(emu["stderr"][ok], 1e-300)).max())
