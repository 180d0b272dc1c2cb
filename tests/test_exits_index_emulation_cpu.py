"""The numpy emulation of the exit-list index and of the ordered adjoints (exits_index_emulation.py) against things that are not
it, without a GPU: the index against a brute-force loop over walks and corners, the ordered sums against math.fsum of the same
terms within the bound the unordered adjoint is documented with (exits_emulation.adjoint_bound: the ordered sum is one of the
orders that bound covers), the gradient form against the float64 scatter of exits_gradient_emulation within ITS bound, exact
zeros for empty bins, and the pieces of the order -- the strided lane sums and the butterfly -- against their definitions."""
import math

import numpy as np
import pytest

import exits_emulation as xe
import exits_gradient_emulation as ge
import exits_index_emulation as xi

INTENSITY = 1.25


def _mesh(rng, n_prims, n_verts, dim):
    return rng.integers(0, n_verts, size=(n_prims, dim)).astype(np.int32)


def _brute_index(rec, prims, n_verts, dim):
    bins = [[] for _ in range(2 * n_verts)]
    n, S = rec["prim"].shape
    for i in range(n):
        for s in range(S):
            if rec["prim"][i, s] < 0:
                continue
            for j in range(dim):
                v = int(prims[rec["prim"][i, s]][j])
                bins[2 * v + (1 if rec["side"][i, s] < 0 else 0)].append((i * S + s) * dim + j)
    return bins


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n,S,n_prims,n_verts,absorbed", [(1, 1, 3, 4, 1.0), (7, 5, 4, 6, 0.7), (40, 9, 3, 12, 0.6), (5, 3, 4, 5, 0.0)])
def test_the_index_against_a_loop_over_walks_and_corners(dim, n, S, n_prims, n_verts, absorbed):
    rng = np.random.default_rng(n * 100 + S)
    prims = _mesh(rng, n_prims, n_verts, dim)
    rec = xe.synthetic_records(rng, n, S, n_prims, dim, absorbed)
    index = xi.build_index(rec, prims, n_verts, dim)
    want = _brute_index(rec, prims, n_verts, dim)
    begin, inc = index["bin_begin"], index["inc"]
    assert begin.dtype == np.int64 and inc.dtype == np.int32 and begin.shape == (2 * n_verts + 1,)
    assert begin[0] == 0 and begin[-1] == len(inc) == dim * int((rec["prim"] >= 0).sum())
    for b in range(2 * n_verts):
        got = inc[begin[b]:begin[b + 1]].tolist()
        assert got == want[b] and got == sorted(got), b
    if absorbed == 0.0:
        assert len(inc) == 0 and np.all(begin == 0)


def test_lane_sums_and_butterfly_are_the_stated_order():
    rng = np.random.default_rng(3)
    t = rng.normal(size=200) * 10.0 ** rng.integers(-8, 8, size=200)
    lanes = xi.lane_sums(t)
    for lane in (0, 7, 8, 63):
        acc = 0.0
        for p in range(lane, 200, 64):
            acc = acc + t[p]
        assert lanes[lane] == acc
    x = lanes.copy()
    for off in (32, 16, 8, 4, 2, 1):
        x = np.array([x[l] + x[l ^ off] for l in range(64)])
    assert xi.butterfly(lanes) == x[0] and np.all(x == x[0])      # (every lane ends with the same bits: + commutes)
    assert xi.butterfly(np.zeros(64)) == 0.0 and not np.signbit(xi.butterfly(np.zeros(64)))
    assert abs(xi.butterfly(lanes) - math.fsum(t)) <= 200 * 2.0 ** -52 * float(np.abs(t).sum())


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n,S,K", [(30, 8, 1), (64, 65, 3)])
def test_the_ordered_adjoint_is_within_the_documented_bound_of_fsum(dim, n, S, K):
    rng = np.random.default_rng(dim * 1000 + n)
    n_prims, n_verts = 5, 9                                   # (some vertex is no corner of any primitive: empty bins)
    prims = _mesh(rng, n_prims, n_verts - 2, dim)
    rec = xe.synthetic_records(rng, n, S, n_prims, dim)
    v = rng.normal(size=(K, n, 3)).astype(np.float32)
    index = xi.build_index(rec, prims, n_verts, dim)
    got = xi.adjoint_ordered(rec, index, v, INTENSITY, dim)
    assert got.shape == (K, n_verts, 6) and got.dtype == np.float32
    emu = xe.adjoint(rec, v, prims, n_verts, INTENSITY, dim)
    # math.fsum of the same terms, entry by entry
    wgt = xe.weights(rec, dim).reshape(-1, dim).astype(np.float64)
    thp = rec["thp"].reshape(-1).astype(np.float64)
    begin, inc = index["bin_begin"], index["inc"].astype(np.int64)
    exact = np.zeros((K, n_verts, 6))
    for k in range(K):
        for b in range(2 * n_verts):
            for c in range(3):
                terms = [float(v[k, (i // dim) // S, c]) / float(S) * float(np.float32(INTENSITY)) * thp[i // dim] * wgt[i // dim, i % dim]
                         for i in inc[begin[b]:begin[b + 1]]]
                exact[k, b >> 1, 3 * (b & 1) + c] = math.fsum(terms)
                assert len(terms) == emu["terms"][k, b >> 1, 3 * (b & 1) + c]
    assert np.all(np.abs(got.astype(np.float64) - exact) <= xe.adjoint_bound(emu))
    empty = emu["terms"] == 0
    assert empty.any() and (emu["terms"] > (128 if S == 65 else 1)).any()      # (bins past a lane's second trip at S = 65)
    assert np.all(got[empty] == 0.0) and not np.signbit(got[empty]).any()
    assert np.all(got[~empty] != 0.0)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("S", [2, 8, 65])
def test_the_ordered_adjoint_of_the_gradient_is_within_its_documented_bound(dim, S):
    rng = np.random.default_rng(dim * 77 + S)
    n, K, n_prims, n_verts, eps = 40, 2, 5, 9, 1e-3
    prims = _mesh(rng, n_prims, n_verts - 2, dim)
    rec, grec = ge.synthetic(rng, n, S, n_prims, dim)
    grec["radius"][3] = 5e-4                                  # degenerate: inside the shell
    grec["radius"][11] = np.nan                               # a point that is not finite
    grec["dirs"][11] = np.nan
    dgrad = rng.normal(size=(K, n, dim, 3)).astype(np.float32)
    dgrad[:, 3] = np.nan                                      # ... whose dgrad is not read
    index = xi.build_index(rec, prims, n_verts, dim)
    got = xi.adjoint_gradient_ordered(rec, grec, index, dgrad, INTENSITY, eps, dim)
    emu = ge.adjoint(rec, grec, np.nan_to_num(dgrad), prims, n_verts, INTENSITY, eps, dim)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got.astype(np.float64) - emu["value"]) <= ge.adjoint_bound(emu))
    assert np.all(got[emu["terms"] == 0] == 0.0) and (emu["terms"] == 0).any()
    # nbar in the stated order is the mean direction to within S roundings
    ok = ~ge.degenerate(grec["radius"], eps) & np.isfinite(grec["radius"])
    mean = grec["dirs"].astype(np.float64).sum(axis=1) / S
    assert np.all(np.abs(xi.nbar(grec["dirs"])[ok] - mean[ok]) <= S * 2.0 ** -52)
