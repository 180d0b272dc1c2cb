"""The index of an exit list and the ordered adjoints in numpy (a helper of the tests, not a test): what wost_exits_index,
wost_exits_adjoint_ordered and wost_exits_adjoint_gradient_ordered compute from a set of records, in the very order
include/wost.h ("Exit lists: the index and the ordered adjoint") states, so that the float32 results are the library's bit for
bit.

A record set `rec` and a gradient part `grec` are the dicts of exits_emulation.py and exits_gradient_emulation.py; `prims` is the
caller's segment / triangle array.

The terms are those of exits_emulation.adjoint and of the contract of the gradient's adjoint, every factor a float64 made from a
float32, the products taken from left to right (numpy rounds each float64 operation once, as the device does with contraction
off).  The order: the entries of a bin at positions lane, lane + 64, ... are added, in that order, to the lane's sum, which
starts at +0.0; the 64 sums go through the butterfly of wave_sum -- x[l] = x[l] + x[l ^ off] for off = 32, 16, 8, 4, 2, 1, every
level one explicit pairwise add --; lane 0's number is cast to float32 once."""
import numpy as np

import exits_emulation as xe
import exits_gradient_emulation as ge

F32 = np.float32
LANES = 64
_LANE = np.arange(LANES)


def build_index(rec, prims, n_verts, dim):
    """-> {"bin_begin" (2 n_verts + 1,) int64, "inc" (n_incidences,) int32}: incidence w * dim + j of absorbed walk w = i * S + s
    and corner j in bin 2 * prims[prim][j] + (side < 0), a bin's incidences ascending"""
    prim, side = rec["prim"].reshape(-1), rec["side"].reshape(-1)
    w = np.nonzero(prim >= 0)[0]
    inc = (w[:, None] * dim + np.arange(dim)[None]).reshape(-1)                                      # ascending
    bins = (2 * np.asarray(prims).reshape(-1, dim)[prim[w]] + (side[w] < 0)[:, None]).reshape(-1)
    order = np.argsort(bins, kind="stable")
    begin = np.zeros(2 * n_verts + 1, np.int64)
    np.cumsum(np.bincount(bins, minlength=2 * n_verts), out=begin[1:])
    return {"bin_begin": begin, "inc": inc[order].astype(np.int32)}


def butterfly(x):
    """the wave_sum of 64 float64 lane values (axis 0), as lane 0 ends up with it: six levels of pairwise adds"""
    x = np.array(x, np.float64)
    assert x.shape[0] == LANES
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[_LANE ^ off]
    return x[0]


def lane_sums(terms):
    """terms (m, ...) float64 in the order of their positions -> (64, ...): lane l's sum of the terms at l, l + 64, ..., from +0.0"""
    terms = np.asarray(terms, np.float64)
    acc = np.zeros((LANES,) + terms.shape[1:])
    for p in range(0, len(terms), LANES):
        chunk = terms[p:p + LANES]
        acc[:len(chunk)] = acc[:len(chunk)] + chunk
    return acc


def nbar(dirs):
    """the mean direction of every point, (n, dim) float64 from (n, S, dim) float32: per-lane strided sums, the butterfly, / S"""
    d = np.asarray(dirs, F32).astype(np.float64)
    S = d.shape[1]
    return np.stack([butterfly(lane_sums(d[i])) / float(S) for i in range(len(d))]) if len(d) else np.zeros((0, d.shape[2]))


def _gather(index, terms_of, K, n_verts):
    """dcolors (K, n_verts, 6) float32 and the terms per entry: terms_of(k, inc) -> (len(inc), 3) float64 in the order given"""
    begin, inc = index["bin_begin"], index["inc"].astype(np.int64)
    out = np.zeros((K, n_verts, 6), F32)
    for k in range(K):
        for b in range(2 * n_verts):
            mine = inc[begin[b]:begin[b + 1]]
            total = butterfly(lane_sums(terms_of(k, mine)))
            out[k, b >> 1, 3 * (b & 1):3 * (b & 1) + 3] = total.astype(F32)
    return out


def adjoint_ordered(rec, index, dfield, intensity, dim):
    """wost_exits_adjoint_ordered: (K, n_verts, 6) float32"""
    d = np.ascontiguousarray(dfield, F32).astype(np.float64)
    d = d[None] if d.ndim == 2 else d
    S = rec["prim"].shape[1]
    wgt = xe.weights(rec, dim).reshape(-1, dim).astype(np.float64)
    thp = rec["thp"].reshape(-1).astype(np.float64)

    def terms(k, inc):
        w, j = inc // dim, inc % dim
        g = d[k, w // S, :] / float(S) * float(F32(intensity)) * thp[w][:, None]
        return g * wgt[w, j][:, None]
    return _gather(index, terms, len(d), (len(index["bin_begin"]) - 1) // 2)


def adjoint_gradient_ordered(rec, grec, index, dgrad, intensity, eps, dim):
    """wost_exits_adjoint_gradient_ordered: (K, n_verts, 6) float32.  An incidence of a degenerate point is skipped: its lane's
    sum stays as it was, and the other incidences keep their positions and lanes"""
    d = np.ascontiguousarray(dgrad, F32).astype(np.float64)
    d = d[None] if d.ndim == 3 else d
    S = rec["prim"].shape[1]
    wgt = xe.weights(rec, dim).reshape(-1, dim).astype(np.float64)
    thp = rec["thp"].reshape(-1).astype(np.float64)
    R = np.asarray(grec["radius"], F32)
    deg = ge.degenerate(R, eps)
    n64 = np.asarray(grec["dirs"], F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        mean = nbar(grec["dirs"])
        cen = (n64 - mean[:, None, :]).reshape(-1, dim)                   # (n * S, dim)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = float(dim) / (R.astype(np.float64) * (float(S) - 1.0))

    def terms(k, inc):
        w, j = inc // dim, inc % dim
        i = w // S
        with np.errstate(invalid="ignore"):
            q = d[k, i, 0, :] * scale[i][:, None] * cen[w, 0][:, None]
            for a in range(1, dim):
                q = q + d[k, i, a, :] * scale[i][:, None] * cen[w, a][:, None]
            t = q * float(F32(intensity)) * thp[w][:, None] * wgt[w, j][:, None]
        return t, deg[i]

    begin, inc = index["bin_begin"], index["inc"].astype(np.int64)
    n_verts = (len(begin) - 1) // 2
    out = np.zeros((len(d), n_verts, 6), F32)
    for k in range(len(d)):
        for b in range(2 * n_verts):
            t, skip = terms(k, inc[begin[b]:begin[b + 1]])
            acc = np.zeros((LANES, 3))
            for p in range(len(t)):
                if not skip[p]:
                    acc[p % LANES] = acc[p % LANES] + t[p]
            out[k, b >> 1, 3 * (b & 1):3 * (b & 1) + 3] = butterfly(acc).astype(F32)
    return out
