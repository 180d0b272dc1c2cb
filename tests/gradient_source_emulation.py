"""The in-ball term of the gradient on a scene with a source term (include/wost.h "The gradient on a scene with a source term",
DESIGN 4.3f "The in-ball term") in numpy on top of the unchanged oracle.  No tests here: test_gradient_source_cpu.py checks the
emulation against closed forms, test_gpu_gradient_source.py the library against the emulation.

The oracle has no gradient and no in-ball term, but everything the term is made of: the PCG32 stream (continued behind the
direction draws of gradient_emulation.directions), sincos_2pi and logf, and the source value -- in 3-D through source_eval3, in
2-D through the identity gradient_emulation.walks uses for walks: the source rendered on a 1 x 1 frame by a zero-scale probe at
y is the source at y.  Item 2 of the header (the samples) is numpy float32 in the written order, item 3 (the reduction) float64.
It combines with gradient_emulation.emulate for the walk part (combine)."""
import ctypes as C

import numpy as np

from oracle.oracle import Settings as _Settings, _fp

_SAMPLES = {}


def _source_at(oracle, sd, dim):
    """y (k, dim) float32 -> the source there (k, 3) float32, intensity included"""
    if dim == 3:
        return lambda y: oracle.source_eval3(sd, y)
    sc = oracle.make_scene({"probe": (0.0, 0.0, 0.0, 0.0, 1.0), "source": sd["source"]})
    keep = list(oracle._keep)      # the scene points into these arrays
    st, one = _Settings(1, 1, 1, 1, 1.0), np.zeros((1, 3), np.float32)

    def at(y):
        out = np.zeros((len(y), 3), np.float32)
        for k in range(len(y)):
            sc.probe_pos[0], sc.probe_pos[1] = float(y[k, 0]), float(y[k, 1])
            assert oracle.lib.wo_render_source(C.byref(sc), C.byref(st), _fp(one)) == 0
            out[k] = one[0]
        return out

    at.keep = keep
    return at


def draws(oracle, i, S, seed_base, seed_width, dim):
    """the S in-ball samples' draws of point i: (S, dim) floats from the stream of pixel seed_base + i, behind the S direction
    draws of dim - 1 floats each -- per sample the dim - 1 floats of the direction, then rho"""
    r = oracle.pcg_seed_pixel(seed_base + i, seed_width)
    for _ in range((dim - 1) * S):
        oracle.pcg_float(r)
    return np.array([oracle.pcg_float(r) for _ in range(dim * S)], np.float32).reshape(S, dim)


def directions(oracle, u, dim):
    """m (S, dim) float32 from a sample's dim - 1 floats, as gradient_emulation.directions forms a walk's direction"""
    one, two = np.float32(1), np.float32(2)
    cs = oracle.probe("sincos_2pi", np.ascontiguousarray(u[:, dim - 2]))
    if dim == 2:
        return cs.astype(np.float32)
    z = one - two * u[:, 0]
    rr = np.sqrt(one - z * z)
    return np.stack([rr * cs[:, 0], rr * cs[:, 1], z], 1).astype(np.float32)


def weights(oracle, rho, dim):
    """(wg, wu) float32 of item 2"""
    one = np.float32(1)
    if dim == 2:
        wu = np.zeros_like(rho)
        pos = rho > 0
        wu[pos] = -(rho[pos] * oracle.probe("logf", np.ascontiguousarray(rho[pos])))
        return one - rho * rho, wu
    return one - (rho * rho) * rho, rho - rho * rho


def samples(oracle, key, sd, pts, R, excluded, S, seed_base, seed_width, dim):
    """item 2 for every point: m (n, S, dim), wg, wu (n, S), ds, ms (n, S, 3) in float32; an excluded point (degenerate, not
    selected, not finite) draws nothing and has zeros.  Cached by key and arguments."""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, dim)
    ck = (key, pts.tobytes(), np.asarray(R, np.float32).tobytes(), np.asarray(excluded).tobytes(), S, seed_base, seed_width, dim)
    if ck in _SAMPLES:
        return _SAMPLES[ck]
    n, half = len(pts), np.float32(0.5)
    out = {"m": np.zeros((n, S, dim), np.float32), "wg": np.zeros((n, S), np.float32), "wu": np.zeros((n, S), np.float32),
           "ds": np.zeros((n, S, 3), np.float32), "ms": np.zeros((n, S, 3), np.float32)}
    source = _source_at(oracle, sd, dim)
    for i in range(n):
        if excluded[i]:
            continue
        u = draws(oracle, i, S, seed_base, seed_width, dim)
        m, rho = directions(oracle, u, dim), u[:, dim - 1]
        r = rho * np.float32(R[i])
        p = r[:, None] * m
        fp, fm = source(pts[i][None, :] + p), source(pts[i][None, :] - p)
        out["m"][i], out["ds"][i], out["ms"][i] = m, half * (fp - fm), half * (fp + fm)
        out["wg"][i], out["wu"][i] = weights(oracle, rho, dim)
    _SAMPLES[ck] = out
    return out


def reduce(smp, R):
    """item 3 in float64: T, seT (n, dim, 3), U (n, 3), the magnitude sums (R / S) sum |a_s|, (R^2 / S) sum |wu ms| that the
    tolerances for fp64 sums in any order take, and seU, the standard error of U (no output of the library: for the checks of
    the emulation itself)"""
    S = smp["m"].shape[1]
    R64 = np.asarray(R, np.float32).astype(np.float64)
    a = smp["wg"].astype(np.float64)[:, :, None, None] * smp["m"].astype(np.float64)[:, :, :, None] * smp["ds"].astype(np.float64)[:, :, None, :]
    b = smp["wu"].astype(np.float64)[:, :, None] * smp["ms"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        T = (R64 / S)[:, None, None] * a.sum(axis=1)
        seT = R64[:, None, None] * np.sqrt(((a - a.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (S - 1) / S)
        U = (R64 * R64 / S)[:, None] * b.sum(axis=1)
        mag_T = (R64 / S)[:, None, None] * np.abs(a).sum(axis=1)
        mag_U = (R64 * R64 / S)[:, None] * np.abs(b).sum(axis=1)
        seU = (R64 * R64)[:, None] * np.sqrt(((b - b.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (S - 1) / S)
    return {"T": T, "seT": seT, "U": U, "mag_T": mag_T, "mag_U": mag_U, "seU": seU}


def combine(emu, red):
    """the emulation of the whole call from gradient_emulation.emulate's walk part and reduce()'s in-ball part: the keys that
    gradient_emulation.assert_matches reads, with the bounds widened by 2^-23 (|T| + mag_T) and 2^-23 (|U| + mag_U).  A degenerate
    point took no samples: its T and U are 0 or NaN times 0 and count as 0."""
    ok = ~emu["degenerate"]
    z = lambda a: np.where(ok.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0.0)
    T, seT, U = z(red["T"]), z(red["seT"]), z(red["U"])
    out = dict(emu)
    out["grad"] = emu["grad"] + T                     # (NaN stays NaN)
    out["stderr"] = np.sqrt(emu["stderr"] ** 2 + seT ** 2)
    out["field"] = emu["field"] + U
    out["tol_grad"] = emu["tol_grad"] + 2.0 ** -23 * (np.abs(T) + z(red["mag_T"]))
    out["tol_field"] = emu["tol_field"] + 2.0 ** -23 * (np.abs(U) + z(red["mag_U"]))
    return out
