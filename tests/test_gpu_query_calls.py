"""The batch queries of the C-ABI (wost_closest_point, wost_closest_silhouette, wost_ray_intersect, wost_render_sdf and their
wost3_ forms) on the paths the Python wrappers never take: optional outputs left out, n == 0, the refusals.  Called through
ctypes on small handles (a dozen segments or triangles, an 8 x 8 frame); what a call does return is the oracle's, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import box_problem, cube_scene3

pytestmark = pytest.mark.gpu

D, N, UNKNOWN = 0, 1, 7                    # mesh selectors: WOST_MESH_DIRICHLET, WOST_MESH_NEUMANN, neither
WOST_ERR_INVALID = -1
SENTINEL = 0x5A


class _Dim:
    """one dimension's handle with both meshes, one with the Dirichlet mesh alone, and the oracle's answers"""

    def __init__(self, dim, oracle):
        from elaina_amd import UniformIntegrator, UniformIntegratorSettings, capi
        from elaina_amd.integrator3d import Problem3, UniformIntegrator3
        self.dim, self.pre, self.lib = dim, "wost_" if dim == 2 else "wost3_", capi.load()
        st = UniformIntegratorSettings((8, 8), 1, 4, 1e-3)
        if dim == 2:
            p = box_problem(n_per_side=6, d_sides=(0, 1), n_sides=(2, 3))
            self.meshes = {D: (p.d_verts, p.d_segs), N: (p.n_verts, p.n_segs)}
            self.it = UniformIntegrator(p, st)
            self.it_d = UniformIntegrator(box_problem(n_per_side=3), st)
            self._cp = lambda v, s, pts: oracle.closest_point(v, s, pts, mode=0)
            self._sil, self._ray = oracle.closest_silhouette, oracle.ray_intersect
        else:
            sd = cube_scene3(n=1, d_faces=(0, 1, 2), n_faces=(3, 4, 5))
            self.meshes = {D: (sd["d_verts"], sd["d_tris"]), N: (sd["n_verts"], sd["n_tris"])}
            self.it = UniformIntegrator3(Problem3.from_dict(sd), st)
            self.it_d = UniformIntegrator3(Problem3.from_dict(cube_scene3(n=1)), st)
            self._cp, self._sil, self._ray = oracle.closest_point3, oracle.closest_silhouette3, oracle.ray_intersect3
        rng = np.random.default_rng(dim)
        self.pts = rng.uniform(-0.5, 1.5, size=(257, dim)).astype(np.float32)
        d = rng.normal(size=(257, dim))
        self.dirs = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
        self.tmax = rng.uniform(0.1, 3.0, 257).astype(np.float32)
        self.rmax = rng.uniform(0.05, 1.0, 257).astype(np.float32)
        # computed once, read by every test of the dimension
        self.cp_ref = {w: self._cp(*self.meshes[w], self.pts) for w in (D, N)}
        self.sil_ref = {r: self._sil(*self.meshes[N], self.pts, self.rmax if r else None) for r in (False, True)}

    def fn(self, name):
        return getattr(self.lib, self.pre + name)

    def error(self):
        return self.lib.wost_last_error().decode()

    def close(self):
        self.it.close()
        self.it_d.close()


@pytest.fixture(scope="module", params=[2, 3], ids=["2d", "3d"])
def dim(request, oracle):
    d = _Dim(request.param, oracle)
    yield d
    d.close()


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _sentinels(dim, n):
    """the four outputs of closest_point for n points, every byte the sentinel"""
    shapes = {"idx": ((n,), np.int32), "dist": ((n,), np.float32), "uv": ((n,) if dim == 2 else (n, 2), np.float32), "side": ((n,), np.int32)}
    return {k: np.frombuffer(bytes([SENTINEL]) * (int(np.prod(s)) * 4), dtype=t).reshape(s).copy() for k, (s, t) in shapes.items()}


def _untouched(a):
    return bool(np.all(a.view(np.uint8) == SENTINEL))


def _closest_point(dim, handle, which, n, out):
    return dim.fn("closest_point")(handle._handle, which, _fp(dim.pts), n, _ip(out.get("idx")), _fp(out.get("dist")), _fp(out.get("uv")),
                                   _ip(out.get("side")))


@pytest.mark.parametrize("n", [1, 256, 257])
@pytest.mark.parametrize("left_out", ["idx", "dist", "uv", "side", "all", "none"])
def test_closest_point_optional_outputs(dim, n, left_out):
    keys = ("idx", "dist", "uv", "side")
    for which in (D, N):
        out = {k: v for k, v in _sentinels(dim.dim, n).items() if left_out not in (k, "all")}
        assert _closest_point(dim, dim.it, which, n, out) == 0, dim.error()
        for k, ref in zip(keys, dim.cp_ref[which]):
            if k in out:
                assert np.array_equal(out[k], ref[:n]), (which, k)


@pytest.mark.parametrize("with_rmax", [False, True])
def test_closest_silhouette_with_and_without_rmax(dim, with_rmax):
    out = np.zeros(257, np.float32)
    rc = dim.fn("closest_silhouette")(dim.it._handle, N, _fp(dim.pts), _fp(dim.rmax if with_rmax else None), 257, _fp(out))
    assert rc == 0, dim.error()
    assert np.array_equal(out, dim.sil_ref[with_rmax])
    assert np.isfinite(out).any()
    if with_rmax:
        assert not np.array_equal(out, dim.sil_ref[False])          # (the bound does cut some answers off)


def _query_calls(dim, handle, which, n):
    """every query with an n: (name, sentinel-filled outputs, the call's return code)"""
    cp = _sentinels(dim.dim, 4)
    sil = _sentinels(dim.dim, 4)["dist"]
    ray = _sentinels(dim.dim, 4)
    return [("closest_point", list(cp.values()), _closest_point(dim, handle, which, n, cp), dim.error()),
            ("closest_silhouette", [sil], dim.fn("closest_silhouette")(handle._handle, which, _fp(dim.pts), _fp(dim.rmax), n, _fp(sil)), dim.error()),
            ("ray_intersect", [ray["idx"], ray["dist"], ray["side"]],
             dim.fn("ray_intersect")(handle._handle, which, _fp(dim.pts), _fp(dim.dirs), _fp(dim.tmax), n, _ip(ray["idx"]), _fp(ray["dist"]),
                                     _ip(ray["side"])), dim.error())]


def test_no_points_is_ok_and_writes_nothing(dim):
    for which in (D, N):
        for name, outs, rc, _ in _query_calls(dim, dim.it, which, 0):
            assert rc == 0, (name, which)
            assert all(_untouched(a) for a in outs), (name, which)


def test_unknown_mesh_selector_is_refused(dim):
    for n in (0, 4):
        for name, outs, rc, msg in _query_calls(dim, dim.it, UNKNOWN, n):
            assert rc == WOST_ERR_INVALID, (name, n)
            assert "unknown" in msg, (name, msg)
            assert all(_untouched(a) for a in outs), (name, n)
    sdf = np.frombuffer(bytes([SENTINEL]) * (64 * 4), dtype=np.float32).copy()
    assert dim.fn("render_sdf")(dim.it._handle, UNKNOWN, _fp(sdf)) == WOST_ERR_INVALID
    assert "unknown mesh selector" in dim.error() and _untouched(sdf)


def test_closest_point_on_an_empty_mesh_is_refused(dim):
    for n in (0, 4):
        out = _sentinels(dim.dim, 4)
        assert _closest_point(dim, dim.it_d, N, n, out) == WOST_ERR_INVALID
        assert "mesh is empty" in dim.error()
        assert all(_untouched(a) for a in out.values())
    # ... while the silhouette and ray queries answer on it: nothing there
    sil = np.zeros(4, np.float32)
    assert dim.fn("closest_silhouette")(dim.it_d._handle, N, _fp(dim.pts), None, 4, _fp(sil)) == 0, dim.error()
    assert np.all(np.isinf(sil))
    hit, t, idx = np.ones(4, np.int32), np.zeros(4, np.float32), np.zeros(4, np.int32)
    assert dim.fn("ray_intersect")(dim.it_d._handle, N, _fp(dim.pts), _fp(dim.dirs), _fp(dim.tmax), 4, _ip(hit), _fp(t), _ip(idx)) == 0, dim.error()
    assert np.all(hit == 0)
