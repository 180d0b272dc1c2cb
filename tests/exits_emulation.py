"""The exit list in numpy (a helper of the tests, not a test): what wost_exits_apply and wost_exits_adjoint compute from a set of
records, operation by operation as include/wost.h ("Exit lists") states them, and the bounds the GPU tests hold the library to.

A record set is the dict exits_records() returns: "prim" (n, S), "uv" (n, S, dim - 1), "side" (n, S), "thp" (n, S), "base"
(n, S, 3).  `prims` is the caller's segment / triangle array (n_prims, dim) and a set of colours is (n_verts, 6).

apply is fp32 per walk (numpy float32 rounds every operation once, as the device does with contraction off) and fp64 per point;
adjoint is fp64 throughout.  The bounds, none of them measured:
  field   an fp64 sum of S terms in any order, one division, one rounding to fp32:  2^-24 |field| + S 2^-52 mean|W|
  stderr  the same for the S squared deviations, which carry the error of the mean twice, under a square root:  relative
          2 S 2^-52 + 2^-23
  adjoint an fp64 sum of M terms in any order, one rounding:  M 2^-52 sum|terms| + 2^-24 |value|"""
import numpy as np

F32 = np.float32


def weights(rec, dim):
    """the fp32 weights of the primitive's vertices, (n, S, dim): (1 - uv, uv) and (1 - u - v, u, v)"""
    uv = rec["uv"].astype(F32)
    if dim == 2:
        return np.stack([F32(1) - uv[..., 0], uv[..., 0]], -1)
    return np.stack([F32(1) - uv[..., 0] - uv[..., 1], uv[..., 0], uv[..., 1]], -1)


def walk_values(rec, colors, prims, intensity, dim):
    """W of every walk for one set of colours, (n, S, 3) float32"""
    colors = np.ascontiguousarray(colors, F32).reshape(-1, 6)
    hit = rec["prim"] >= 0
    verts = np.asarray(prims).reshape(-1, dim)[np.where(hit, rec["prim"], 0)]          # (n, S, dim)
    off = np.where(rec["side"] >= 0, 0, 3)
    w = weights(rec, dim)
    W = rec["base"].astype(F32).copy()
    for c in range(3):
        cols = [colors[verts[..., v], off + c] for v in range(dim)]
        with np.errstate(invalid="ignore"):
            col = cols[0] * w[..., 0] + cols[1] * w[..., 1]
            if dim == 3:
                col = col + cols[2] * w[..., 2]
            col = col * F32(intensity)
            col = col * rec["thp"].astype(F32)
            W[..., c] = np.where(hit, col + rec["base"][..., c].astype(F32), rec["base"][..., c])
    assert W.dtype == F32
    return W


def apply(rec, color_sets, prims, intensity, dim):
    """-> {"W": (K, n, S, 3) float32, "mean": (K, n, 3) float64, "field": its float32, "stderr64": (K, n, 3) float64, "stderr":
    its float32}"""
    sets = np.ascontiguousarray(color_sets, F32)
    sets = sets[None] if sets.ndim == 2 else sets
    W = np.stack([walk_values(rec, c, prims, intensity, dim) for c in sets])
    S = W.shape[2]
    W64 = W.astype(np.float64)
    mean = W64.sum(2) / S
    with np.errstate(divide="ignore", invalid="ignore"):
        se = np.sqrt(((W64 - mean[:, :, None]) ** 2).sum(2) / (S - 1) / S) if S > 1 else np.full(mean.shape, np.inf)
    return {"W": W, "mean": mean, "field": mean.astype(F32), "stderr64": se, "stderr": se.astype(F32)}


def field_bound(emu):
    S = emu["W"].shape[2]
    return 2.0 ** -24 * np.abs(emu["mean"]) + S * 2.0 ** -52 * np.abs(emu["W"].astype(np.float64)).mean(2)


def stderr_rel_bound(S):
    return 2.0 * S * 2.0 ** -52 + 2.0 ** -23


def adjoint(rec, dfield, prims, n_verts, intensity, dim):
    """-> {"value": (K, n_verts, 6) float64, "abs": the sum of |terms| per entry, "terms": their number M}"""
    d = np.ascontiguousarray(dfield, np.float64)
    d = d[None] if d.ndim == 2 else d
    K, n = d.shape[:2]
    S = rec["prim"].shape[1]
    out = {"value": np.zeros((K, n_verts, 6)), "abs": np.zeros((K, n_verts, 6)), "terms": np.zeros((K, n_verts, 6), np.int64)}
    hit = rec["prim"] >= 0
    ii, ss = np.nonzero(hit)
    verts = np.asarray(prims).reshape(-1, dim)[rec["prim"][ii, ss]]                        # (m, dim)
    off = np.where(rec["side"][ii, ss] >= 0, 0, 3)
    w = weights(rec, dim)[ii, ss].astype(np.float64)
    thp = rec["thp"][ii, ss].astype(np.float64)
    for k in range(K):
        for c in range(3):
            g = d[k, ii, c] / float(S) * float(F32(intensity)) * thp
            for v in range(dim):
                t = g * w[:, v]
                np.add.at(out["value"][k], (verts[:, v], off + c), t)
                np.add.at(out["abs"][k], (verts[:, v], off + c), np.abs(t))
                np.add.at(out["terms"][k], (verts[:, v], off + c), 1)
    return out


def adjoint_bound(emu):
    return emu["terms"] * 2.0 ** -52 * emu["abs"] + 2.0 ** -24 * np.abs(emu["value"])


def synthetic_records(rng, n, S, n_prims, dim, absorbed=0.7):
    """random records with every kind of walk in them: absorbed on either side, not absorbed"""
    hit = rng.uniform(size=(n, S)) < absorbed
    uv = rng.uniform(0.05, 0.45, size=(n, S, dim - 1)).astype(F32)
    return {"prim": np.where(hit, rng.integers(0, n_prims, size=(n, S)), -1).astype(np.int32),
            "uv": np.where(hit[..., None], uv, 0).astype(F32),
            "side": np.where(hit, rng.choice([-1, 0, 1], size=(n, S)), 0).astype(np.int32),
            "thp": rng.uniform(0.5, 1.5, size=(n, S)).astype(F32),
            "base": rng.normal(size=(n, S, 3)).astype(F32)}
