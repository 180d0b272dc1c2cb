"""The exit list of the gradient in numpy (a helper of the tests, not a test): what wost_exits_apply_gradient and
wost_exits_adjoint_gradient compute from a set of records, as include/wost.h ("Exit lists of the gradient") states them, and the
bounds the GPU tests hold the library to.

A list is two dicts: `rec`, what exits_records() returns (exits_emulation.py), and `grec`, what exits_gradient_records()
returns -- "radius" (n,), "dirs" (n, S, dim), "first_pts" (n, S, dim), float32.  `prims` is the caller's segment / triangle
array and a set of colours is (n_verts, 6).

apply: W per walk through exits_emulation.walk_values (float32, operation by operation), then the reduction of the gradient's
contract (item 4) in float64.  adjoint: a float64 scatter.  linear: the linear part J c of apply in float64 throughout, which is
what the adjoint transposes.

The bound of the adjoint, derived, not measured.  With u = 2^-53 (an fp64 rounding), an entry of M terms, S walks per point:
  - a term is  t = q * intensity * thp * w_v  with  q = sum_axis dgrad_axis * scale * (n_axis - nbar_axis)  and  scale = DIM /
    (R (S - 1)).  Let  a = sum_axis |dgrad_axis| * scale * intensity * thp * w_v  be the term without its direction factor.
    |n - nbar| <= 2, so |t| <= 2 a.
  - nbar is an fp64 sum of S numbers of size <= 1 in any order, divided by S: its error is at most (S - 1) u + u <= S u.  The
    difference n - nbar adds one rounding, u |n - nbar| <= 2 u.  So the direction factor is off by at most (S + 2) u in absolute
    terms, which moves t by at most (S + 2) u a.
  - scale takes 3 roundings, each product of an axis 2, the DIM - 1 additions of the axes one each, the three last factors 3: at
    most 8 + DIM <= 11 roundings relative to a number no larger than 2 a, so 22 u a.
  - the sum of M such terms in any order: (M - 1) u sum |t| <= M u sum 2 a.
  Together one evaluation is within  [M + (S + 2) / 2 + 11] u sum 2 a  of the exact value.  The library and this module each
  make one evaluation, in different orders, so they differ by at most twice that:  (M + S / 2 + 12) 2^-52 sum 2 a.  The library
  then rounds to fp32 once: 2^-24 |value|.  adjoint_bound() uses  (M + S + 12) 2^-52 sum 2 a + 2^-24 |value|  -- the S of the
  expected form (the order of the nbar sum) kept whole, and 12 where a count without the roundings of scale and of the axes
  would have 8."""
import numpy as np

import exits_emulation as xe

F32 = np.float32


def degenerate(radius, eps):
    R = np.asarray(radius, F32)
    return ~(R > F32(eps)) | ~np.isfinite(R)


def reduce(W, dirs, radius, eps, dim):
    """item 4 of the gradient's contract in float64 from float32 W (n, S, 3), directions (n, S, dim) and radii (n,) -> grad and
    stderr (n, dim, 3), field (n, 3); a degenerate point: NaN, NaN and its mean"""
    S = W.shape[1]
    W64, n64, R64 = W.astype(np.float64), dirs.astype(np.float64), np.asarray(radius, np.float64)[:, None, None]
    mean = W64.sum(axis=1) / S
    t = n64[:, :, :, None] * (W64 - mean[:, None, :])[:, :, None, :]          # (n, S, dim, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = dim / (R64 * (S - 1)) * t.sum(axis=1)
        se = dim / R64 * np.sqrt(((t - t.sum(axis=1, keepdims=True) / S) ** 2).sum(axis=1) / (S - 1) / S)
    deg = degenerate(radius, eps)
    grad[deg] = se[deg] = np.nan
    return grad, se, mean


def apply(rec, grec, color_sets, prims, intensity, eps, dim):
    """-> {"W": (K, n, S, 3) float32, "grad", "stderr": (K, n, dim, 3) float64, "field": (K, n, 3) float64}"""
    sets = np.ascontiguousarray(color_sets, F32)
    sets = sets[None] if sets.ndim == 2 else sets
    W = np.stack([xe.walk_values(rec, c, prims, intensity, dim) for c in sets])
    parts = [reduce(w, grec["dirs"], grec["radius"], eps, dim) for w in W]
    return {"W": W, "grad": np.stack([p[0] for p in parts]), "stderr": np.stack([p[1] for p in parts]), "field": np.stack([p[2] for p in parts])}


def _terms(rec, grec, prims, intensity, eps, dim):
    """what apply's linear part and the adjoint share, over the absorbed walks of non-degenerate points, float64: their point and
    walk, vertices (m, dim), side offset, the factor intensity * thp * w_v (m, dim), scale (m,) and n - nbar (m, dim)"""
    S = rec["prim"].shape[1]
    n64 = grec["dirs"].astype(np.float64)
    centred = n64 - n64.sum(axis=1, keepdims=True) / S
    ok = (rec["prim"] >= 0) & ~degenerate(grec["radius"], eps)[:, None]
    ii, ss = np.nonzero(ok)
    verts = np.asarray(prims).reshape(-1, dim)[rec["prim"][ii, ss]]
    off = np.where(rec["side"][ii, ss] >= 0, 0, 3)
    w = xe.weights(rec, dim)[ii, ss].astype(np.float64)
    factor = float(F32(intensity)) * rec["thp"][ii, ss].astype(np.float64)[:, None] * w
    scale = dim / (grec["radius"].astype(np.float64)[ii] * (S - 1))
    return ii, verts, off, factor, scale, centred[ii, ss]


def linear(rec, grec, color_sets, prims, intensity, eps, dim):
    """J c, the part of grad that is linear in the colours, (K, n, dim, 3) float64 -- apply(c) - apply(0) without the fp32
    rounding of W; a degenerate point: zeros (it adds nothing to the adjoint either)"""
    sets = np.ascontiguousarray(color_sets, np.float64)
    sets = sets[None] if sets.ndim == 2 else sets
    n = rec["prim"].shape[0]
    ii, verts, off, factor, scale, centred = _terms(rec, grec, prims, intensity, eps, dim)
    out = np.zeros((len(sets), n, dim, 3))
    for k, colors in enumerate(sets):
        for c in range(3):
            col = sum(colors[verts[:, v], off + c] * factor[:, v] for v in range(dim))          # (m,)
            for axis in range(dim):
                np.add.at(out[k, :, axis, c], ii, scale * centred[:, axis] * col)
    return out


def adjoint(rec, grec, dgrad, prims, n_verts, intensity, eps, dim):
    """-> {"value": (K, n_verts, 6) float64, "abs": the sum of 2 a per entry (a: the term without its direction factor), "terms":
    their number M, "S"}"""
    d = np.ascontiguousarray(dgrad, np.float64)
    d = d[None] if d.ndim == 3 else d
    K = d.shape[0]
    ii, verts, off, factor, scale, centred = _terms(rec, grec, prims, intensity, eps, dim)
    out = {"value": np.zeros((K, n_verts, 6)), "abs": np.zeros((K, n_verts, 6)), "terms": np.zeros((K, n_verts, 6), np.int64),
           "S": rec["prim"].shape[1]}
    for k in range(K):
        for c in range(3):
            q = sum(d[k, ii, axis, c] * scale * centred[:, axis] for axis in range(dim))
            a = sum(np.abs(d[k, ii, axis, c]) * scale for axis in range(dim))
            for v in range(dim):
                np.add.at(out["value"][k], (verts[:, v], off + c), q * factor[:, v])
                np.add.at(out["abs"][k], (verts[:, v], off + c), 2.0 * a * np.abs(factor[:, v]))
                np.add.at(out["terms"][k], (verts[:, v], off + c), 1)
    return out


def adjoint_bound(emu):
    return (emu["terms"] + emu["S"] + 12) * 2.0 ** -52 * emu["abs"] + 2.0 ** -24 * np.abs(emu["value"])


def identity_slack(emu):
    """what the float64 evaluation of <dgrad, J c> may itself be off by, per unit of |c| of an entry: J c sums the same products
    as the adjoint, entry by entry of c, so the derivation above holds for it with its own orders"""
    return (emu["terms"] + emu["S"] + 12) * 2.0 ** -52 * emu["abs"]


def synthetic(rng, n, S, n_prims, dim, absorbed=0.7):
    """random records and a gradient part to go with them: unit directions, radii well above any shell"""
    rec = xe.synthetic_records(rng, n, S, n_prims, dim, absorbed)
    d = rng.normal(size=(n, S, dim))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    grec = {"radius": rng.uniform(0.05, 0.5, size=n).astype(F32), "dirs": d.astype(F32),
            "first_pts": rng.uniform(size=(n, S, dim)).astype(F32)}
    return rec, grec
