"""The numpy emulation of the exit list (exits_emulation.py) on synthetic records, without a GPU: apply and adjoint are transposes
of one another, a walk that was not absorbed contributes its base and nothing else, the side picks the colour triple, and one
walk per point has no error estimate."""
import numpy as np
import pytest

import exits_emulation as xe

INTENSITY = 1.25


def _scene(rng, dim, n_verts=23, n_prims=17):
    prims = np.stack([rng.permutation(n_verts)[:dim] for _ in range(n_prims)]).astype(np.int32)
    return prims, n_verts


@pytest.mark.parametrize("dim", [2, 3])
def test_apply_and_adjoint_are_transposes(dim):
    """sum field * v == sum colors * adjoint(v) + (the part of field that no colour reaches) * v, to fp64 rounding: the map is
    affine in the colours, so the identity is taken on the difference of two colour sets, where the bases cancel.  apply forms W
    in fp32, so its linear part is taken in fp64 from the same weights"""
    rng = np.random.default_rng(dim)
    prims, n_verts = _scene(rng, dim)
    rec = xe.synthetic_records(rng, 9, 5, len(prims), dim)
    K, n, S = 3, 9, 5
    colors = rng.normal(size=(K, n_verts, 6)).astype(np.float32)
    v = rng.normal(size=(K, n, 3)).astype(np.float32)
    adj = xe.adjoint(rec, v, prims, n_verts, INTENSITY, dim)
    # the linear part of apply in fp64: field_lin[k][i][c] = sum_s intensity thp sum_v w_v colors[k][v][off + c] / S
    w = xe.weights(rec, dim).astype(np.float64)
    lin = np.zeros((K, n, 3))
    for i in range(n):
        for s in range(S):
            if rec["prim"][i, s] < 0:
                continue
            off = 0 if rec["side"][i, s] >= 0 else 3
            for k in range(K):
                for c in range(3):
                    col = sum(float(colors[k, prims[rec["prim"][i, s], j], off + c]) * w[i, s, j] for j in range(dim))
                    lin[k, i, c] += col * float(np.float32(INTENSITY)) * float(rec["thp"][i, s]) / S
    lhs = float((lin * v.astype(np.float64)).sum())
    rhs = float((colors.astype(np.float64) * adj["value"]).sum())
    scale = float((np.abs(colors.astype(np.float64)) * adj["abs"]).sum())
    assert abs(lhs - rhs) <= 64 * 2.0 ** -52 * scale, (lhs, rhs)
    # ... and the fp32 apply agrees with that linear part plus the bases to fp32 rounding of each walk
    emu = xe.apply(rec, colors, prims, INTENSITY, dim)
    full = lin + rec["base"].astype(np.float64).sum(1)[None] / S
    assert np.all(np.abs(emu["mean"] - full) <= 8 * 2.0 ** -24 * (np.abs(emu["W"]).max() + 4.0))


@pytest.mark.parametrize("dim", [2, 3])
def test_a_walk_that_was_not_absorbed_contributes_its_base_only(dim):
    rng = np.random.default_rng(10 + dim)
    prims, n_verts = _scene(rng, dim)
    rec = xe.synthetic_records(rng, 6, 4, len(prims), dim, absorbed=0.0)
    assert np.all(rec["prim"] == -1)
    colors = rng.normal(size=(2, n_verts, 6)).astype(np.float32)
    emu = xe.apply(rec, colors, prims, INTENSITY, dim)
    assert np.array_equal(emu["W"][0], rec["base"]) and np.array_equal(emu["W"][1], rec["base"])
    adj = xe.adjoint(rec, rng.normal(size=(2, 6, 3)), prims, n_verts, INTENSITY, dim)
    assert not adj["value"].any() and not adj["terms"].any()
    # a mixed list: vertices of primitives nobody exits at get exactly zero
    rec = xe.synthetic_records(rng, 6, 4, 3, dim, absorbed=0.6)
    adj = xe.adjoint(rec, rng.normal(size=(1, 6, 3)), prims, n_verts, INTENSITY, dim)
    touched = np.zeros(n_verts, bool)
    touched[prims[np.unique(rec["prim"][rec["prim"] >= 0])].reshape(-1)] = True
    assert np.all(adj["value"][0, ~touched] == 0.0) and adj["value"][0, touched].any()


@pytest.mark.parametrize("dim", [2, 3])
def test_the_side_picks_the_colour_triple(dim):
    prims = np.arange(dim, dtype=np.int32)[None]
    uv = np.full((1, 3, dim - 1), 0.25, np.float32)
    rec = {"prim": np.zeros((1, 3), np.int32), "uv": uv, "side": np.array([[1, 0, -1]], np.int32), "thp": np.ones((1, 3), np.float32),
           "base": np.zeros((1, 3, 3), np.float32)}
    colors = np.zeros((dim, 6), np.float32)
    colors[:, 0:3] = (1.0, 2.0, 3.0)       # the side of the normal (side >= 0)
    colors[:, 3:6] = (10.0, 20.0, 30.0)    # the other side
    W = xe.walk_values(rec, colors, prims, 1.0, dim)
    assert np.array_equal(W[0, 0], [1.0, 2.0, 3.0]) and np.array_equal(W[0, 1], [1.0, 2.0, 3.0]) and np.array_equal(W[0, 2], [10.0, 20.0, 30.0])
    d = np.zeros((1, 3), np.float64)
    d[0, 1] = 3.0
    adj = xe.adjoint(rec, d, prims, dim, 1.0, dim)["value"][0]
    # channel 1: two walks on the first triple (column 1), one on the second (column 4); the weights sum to one per walk
    assert abs(adj[:, 1].sum() - 2.0) < 1e-12 and abs(adj[:, 4].sum() - 1.0) < 1e-12
    assert not adj[:, [0, 2, 3, 5]].any()
    # swapped weights or a flipped offset are other numbers
    w = xe.weights(rec, dim)[0, 0]
    assert w[0] == np.float32(0.75) if dim == 2 else w[0] == np.float32(0.5)
    assert np.allclose(adj[:, 1], 2.0 * w) and np.allclose(adj[:, 4], w)


def test_one_walk_per_point_has_an_infinite_standard_error():
    rng = np.random.default_rng(5)
    prims, n_verts = _scene(rng, 2)
    rec = xe.synthetic_records(rng, 4, 1, len(prims), 2)
    emu = xe.apply(rec, rng.normal(size=(2, n_verts, 6)).astype(np.float32), prims, INTENSITY, 2)
    assert np.all(np.isposinf(emu["stderr"])) and np.array_equal(emu["field"], emu["W"][:, :, 0])
    rec = xe.synthetic_records(rng, 4, 2, len(prims), 2)
    emu = xe.apply(rec, rng.normal(size=(1, n_verts, 6)).astype(np.float32), prims, INTENSITY, 2)
    W = emu["W"][0].astype(np.float64)
    assert np.allclose(emu["stderr"][0], np.abs(W[:, 0] - W[:, 1]) / 2.0, rtol=1e-6)
