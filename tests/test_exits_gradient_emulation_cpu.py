"""The numpy emulation of the exit list of the gradient (exits_gradient_emulation.py) on synthetic records, without a GPU: the
properties the GPU tests then lean on -- apply is affine in the colours, its linear part and the adjoint are transposes of one
another, a constant added to every W leaves the gradient alone, and degenerate and non-finite points contribute nothing."""
import numpy as np
import pytest

import exits_emulation as xe
import exits_gradient_emulation as xg

EPS, INTENSITY, N_VERTS, N_PRIMS = 1e-3, 1.25, 30, 40


def _list(dim, seed, n=12, S=9):
    rng = np.random.default_rng(seed)
    rec, grec = xg.synthetic(rng, n, S, N_PRIMS, dim)
    prims = rng.integers(0, N_VERTS, size=(N_PRIMS, dim)).astype(np.int32)
    return rng, rec, grec, prims


def _colors(rng, K=None):
    return rng.uniform(-1.0, 2.0, size=((N_VERTS, 6) if K is None else (K, N_VERTS, 6))).astype(np.float32)


@pytest.mark.parametrize("dim", [2, 3])
def test_apply_is_affine_in_the_colours(dim):
    """apply(c) - apply(0) is the float64 linear part up to the fp32 roundings of W: a walk's W carries at most five of them on
    numbers no larger than |W| + |base|, and grad weighs a walk by scale |n - nbar| <= 2 scale"""
    rng, rec, grec, prims = _list(dim, 1)
    sets = _colors(rng, 3)
    emu, zero = xg.apply(rec, grec, sets, prims, INTENSITY, EPS, dim), xg.apply(rec, grec, np.zeros_like(sets[0]), prims, INTENSITY, EPS, dim)
    lin = xg.linear(rec, grec, sets, prims, INTENSITY, EPS, dim)
    S = rec["prim"].shape[1]
    scale = dim / (grec["radius"].astype(np.float64) * (S - 1))
    size = (np.abs(emu["W"].astype(np.float64)) + np.abs(rec["base"].astype(np.float64))[None]).sum(2)          # (K, n, 3)
    tol = 2.0 * scale[None, :, None, None] * 6 * 2.0 ** -24 * size[:, :, None, :]
    err = np.abs((emu["grad"] - zero["grad"]) - lin)
    assert np.all(err <= tol), float((err / tol).max())
    assert np.abs(lin).max() > 1e4 * tol.max()
    # ... and J itself is linear to fp64 rounding
    a, b = sets[0].astype(np.float64), sets[1].astype(np.float64)
    both = xg.linear(rec, grec, 0.25 * a - 3.0 * b, prims, INTENSITY, EPS, dim)[0]
    assert np.allclose(both, 0.25 * lin[0] - 3.0 * lin[1], rtol=0, atol=1e-12 * np.abs(lin).max())


@pytest.mark.parametrize("dim", [2, 3])
def test_the_linear_part_and_the_adjoint_are_transposes(dim):
    rng, rec, grec, prims = _list(dim, 2)
    K = 2
    sets = _colors(rng, K).astype(np.float64)
    dgrad = rng.normal(size=(K, rec["prim"].shape[0], dim, 3))
    lin = xg.linear(rec, grec, sets, prims, INTENSITY, EPS, dim)
    adj = xg.adjoint(rec, grec, dgrad, prims, N_VERTS, INTENSITY, EPS, dim)
    lhs, rhs = float((dgrad * lin).sum()), float((adj["value"] * sets).sum())
    tol = float((np.abs(sets) * 2.0 * xg.identity_slack(adj)).sum())
    assert abs(lhs - rhs) <= tol and abs(lhs) > 1e6 * tol, (lhs, rhs, tol)
    # every absorbed walk of the list adds dim * 3 terms per set, and no entry without a term has a value
    assert int(adj["terms"].sum()) == int((rec["prim"] >= 0).sum()) * dim * 3 * K
    assert np.all(adj["value"][adj["terms"] == 0] == 0.0) and np.any(adj["terms"] == 0) and np.any(adj["terms"] > 1)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_constant_added_to_every_walk_leaves_the_gradient_alone(dim):
    """sum_s (n_s - nbar) = 0: the centred directions cancel to rounding, and W + const gives the same grad in float64 to the
    rounding of S numbers of the size of the constant"""
    rng, rec, grec, prims = _list(dim, 3)
    S = rec["prim"].shape[1]
    n64 = grec["dirs"].astype(np.float64)
    assert np.abs((n64 - n64.sum(1, keepdims=True) / S).sum(1)).max() <= S * 2.0 ** -52
    W = xe.walk_values(rec, _colors(rng), prims, INTENSITY, dim).astype(np.float64)
    const = 64.0          # exact in every sum with W: |W| < 2^6 and float32 has 24 bits, float64 53
    g0, se0, f0 = xg.reduce(W, grec["dirs"], grec["radius"], EPS, dim)
    g1, se1, f1 = xg.reduce(W + const, grec["dirs"], grec["radius"], EPS, dim)
    scale = dim / (grec["radius"].astype(np.float64) * (S - 1))
    tol = (scale * 4 * S * 2.0 ** -52 * (const + np.abs(W).max()))[:, None, None] * S
    assert np.all(np.abs(g1 - g0) <= tol) and np.all(np.abs(se1 - se0) <= tol) and np.allclose(f1, f0 + const, rtol=0, atol=1e-12)
    assert np.abs(g0).max() > 1e6 * tol.max()


@pytest.mark.parametrize("dim", [2, 3])
def test_degenerate_and_non_finite_points_contribute_nothing(dim):
    rng, rec, grec, prims = _list(dim, 4)
    dgrad = rng.normal(size=(1, rec["prim"].shape[0], dim, 3))
    sets = _colors(rng, 1)
    whole = xg.adjoint(rec, grec, dgrad, prims, N_VERTS, INTENSITY, EPS, dim)
    # point 2 falls into the shell, point 5 has no boundary in reach, point 7 is not finite (as the library records it)
    grec = {k: v.copy() for k, v in grec.items()}
    rec = {k: v.copy() for k, v in rec.items()}
    grec["radius"][2], grec["radius"][5], grec["radius"][7] = 0.5 * EPS, np.inf, np.nan
    grec["dirs"][7] = grec["first_pts"][7] = np.nan
    rec["prim"][7], rec["side"][7], rec["uv"][7] = -1, 0, 0
    rec["thp"][7] = rec["base"][7] = np.nan
    out = (2, 5, 7)
    emu = xg.apply(rec, grec, sets, prims, INTENSITY, EPS, dim)
    assert np.all(np.isnan(emu["grad"][:, out])) and np.all(np.isnan(emu["stderr"][:, out]))
    assert np.all(np.isfinite(emu["field"][:, (2, 5)])) and np.all(np.isnan(emu["field"][:, 7]))
    rest = np.setdiff1d(np.arange(rec["prim"].shape[0]), out)
    assert np.all(np.isfinite(emu["grad"][:, rest]))
    assert np.all(xg.linear(rec, grec, sets, prims, INTENSITY, EPS, dim)[:, out] == 0.0)
    # the adjoint is that of the list without them -- and does not read their dgrad, NaN or not
    dgrad[:, out] = np.nan
    part = xg.adjoint(rec, grec, dgrad, prims, N_VERTS, INTENSITY, EPS, dim)
    keep = {k: v[rest] for k, v in rec.items()}
    gkeep = {k: v[rest] for k, v in grec.items()}
    want = xg.adjoint(keep, gkeep, dgrad[:, rest], prims, N_VERTS, INTENSITY, EPS, dim)
    assert np.array_equal(part["value"], want["value"]) and np.array_equal(part["terms"], want["terms"])
    assert np.all(np.isfinite(part["value"])) and part["terms"].sum() < whole["terms"].sum()
