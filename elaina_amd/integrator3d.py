"""Python mirror of Problem<3> / UniformIntegrator<3> (reference core/problem.h:197-260,
integrator/uniform/integrator.h:55-131 with DIM = 3) on top of the wost3_* entry points of the C-ABI.
Thin ctypes calls into libwost_hip.so -- no arithmetic happens here."""
import ctypes as C

import numpy as np

from . import capi
from .capi import Mesh3Desc, Scene3Desc, Settings, _check, _fp, _ip
from .guided import GuidedCalls, guided_settings
from .uniform import UniformCalls


class Problem3:
    """Triangle meshes + EvaluationGrid<3> probe.  probe = (scale, pos[3], up[3], right[3])
    (core/evaluation_grid.h:48-55); colors [n_verts, 6] = rgb on the normal side, rgb on the other."""

    def __init__(self, d_verts=None, d_tris=None, d_colors=None, n_verts=None, n_tris=None, n_colors=None,
                 probe=(1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), dirichlet_intensity=1.0, neumann_intensity=1.0,
                 mask=None, source=None):
        def arr(a, dt, cols):
            return None if a is None else np.ascontiguousarray(a, dtype=dt).reshape(-1, cols)
        self.d_verts, self.d_tris, self.d_colors = arr(d_verts, np.float32, 3), arr(d_tris, np.int32, 3), arr(d_colors, np.float32, 6)
        self.n_verts, self.n_tris, self.n_colors = arr(n_verts, np.float32, 3), arr(n_tris, np.int32, 3), arr(n_colors, np.float32, 6)
        self.probe = probe
        self.dirichlet_intensity, self.neumann_intensity = float(dirichlet_intensity), float(neumann_intensity)
        self.mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        # source term: {"rgb": [nz, ny, nx, 3], "index_scale": (3,), "index_offset": (3,), "intensity": f} or None
        self.source = None if source is None else dict(source, rgb=np.ascontiguousarray(source["rgb"], dtype=np.float32))

    @classmethod
    def from_dict(cls, sd):
        return cls(**{k: sd.get(k) for k in ("d_verts", "d_tris", "d_colors", "n_verts", "n_tris", "n_colors", "mask", "source")},
                   probe=sd["probe"], dirichlet_intensity=sd.get("dirichlet_intensity", 1.0),
                   neumann_intensity=sd.get("neumann_intensity", 1.0))

    def as_dict(self):
        return {k: getattr(self, k) for k in ("d_verts", "d_tris", "d_colors", "n_verts", "n_tris", "n_colors", "probe",
                                              "dirichlet_intensity", "neumann_intensity", "mask", "source")}


def _mesh3(keep, verts, tris, colors):
    m = Mesh3Desc()
    if verts is None or tris is None or len(tris) == 0:
        return m
    keep += [verts, tris]
    m.n_verts, m.n_tris, m.verts, m.tris = len(verts), len(tris), _fp(verts), _ip(tris)
    if colors is not None:
        if colors.shape != (len(verts), 6):
            raise ValueError("colors must be [n_verts, 6]")
        keep.append(colors)
        m.colors = _fp(colors)
    return m


def scene3_desc(keep, problem, w, h):
    """wost3_scene_desc of a Problem3 (arrays referenced from `keep`)"""
    sc = Scene3Desc()
    sc.dirichlet = _mesh3(keep, problem.d_verts, problem.d_tris, problem.d_colors)
    sc.neumann = _mesh3(keep, problem.n_verts, problem.n_tris, problem.n_colors)
    sc.dirichlet_intensity, sc.neumann_intensity = problem.dirichlet_intensity, problem.neumann_intensity
    scale, pos, up, right = problem.probe
    sc.probe_scale = float(scale)
    for k in range(3):
        sc.probe_pos[k], sc.probe_up[k], sc.probe_right[k] = float(pos[k]), float(up[k]), float(right[k])
    if problem.mask is not None:
        if problem.mask.size != w * h:
            raise ValueError("mask must have width*height entries")
        keep.append(problem.mask)
        sc.mask = problem.mask.ctypes.data_as(C.POINTER(C.c_uint8))
    if problem.source is not None:
        rgb = problem.source["rgb"]
        if rgb.ndim != 4 or rgb.shape[3] != 3:
            raise ValueError("source rgb must be [nz, ny, nx, 3]")
        keep.append(rgb)
        sc.source.nz, sc.source.ny, sc.source.nx = rgb.shape[:3]
        sc.source.rgb = _fp(rgb)
        for k in range(3):
            sc.source.index_scale[k] = float(problem.source["index_scale"][k])
            sc.source.index_offset[k] = float(problem.source["index_offset"][k])
        sc.source.intensity = float(problem.source.get("intensity", 1.0))
    return sc


class UniformIntegrator3(UniformCalls):
    _prefix, _dim = "wost3_", 3      # (UniformCalls: the solves, the carried solve, the batch queries, close)
    VectorType = tuple

    def __init__(self, problem, settings, device=0):
        self.lib = capi.load()
        self.problem, self.settings = problem, settings
        keep = []
        w, h = settings.frameSize
        sc = scene3_desc(keep, problem, w, h)
        st = Settings(w, h, settings.samplesPerPixel, settings.maxWalkingDepth, settings.epsilonShell)
        self._handle = C.c_void_p()
        _check(self.lib.wost3_create(C.byref(sc), C.byref(st), device, C.byref(self._handle)), "wost3_create")
        self.n_pixels = w * h
        self.solution, self.last_stats = None, None

    def set_option(self, key, value):
        """wost3_set_option: "grad_source" 1 lets the gradient calls take a scene with a source term (0, the default: refused);
        "exits_grad_source" 1 lets exits_walk_gradient take one and carry the in-ball term in the list (0, the default: refused)"""
        _check(self.lib.wost3_set_option(self._handle, key.encode(), float(value)), "wost3_set_option")

    def render_sdf(self, which=0):
        """renderDirichletSDF (which = 0) / renderSilhouetteSDF (which = 1): one distance per pixel of the frame"""
        out = np.zeros(self.n_pixels, dtype=np.float32)
        _check(self.lib.wost3_render_sdf(self._handle, int(which), _fp(out)), "wost3_render_sdf")
        return out

    def render_source(self):
        """renderSource: intensity * f at every pixel's evaluation point"""
        out = np.zeros((self.n_pixels, 3), dtype=np.float32)
        _check(self.lib.wost3_render_source(self._handle, _fp(out)), "wost3_render_source")
        return out


MESH_BUILD_ARRAYS = ("nodes", "tri", "triOrig", "slotOfOrig", "triVerts", "colors", "flat", "flatVerts", "edges", "slotEdges", "cones", "obox",
                     "areas", "sampTri", "scalars")


def mesh_build_check(verts, tris, colors=None, repeat=1, device=0):
    """wost3_mesh_build_check: the device build of a triangle mesh against the host builder kept as its checker ->
    ({array: differing bytes}, bytes compared, host ms, device ms)"""
    keep = []
    verts = np.ascontiguousarray(verts, np.float32)
    tris = np.ascontiguousarray(tris, np.int32)
    colors = None if colors is None else np.ascontiguousarray(colors, np.float32)
    m = _mesh3(keep, verts, tris, colors)
    host_ms, dev_ms = C.c_double(0.0), C.c_double(0.0)
    mism = (C.c_int64 * 16)()
    lib = capi.load()
    _check(lib.wost3_mesh_build_check(C.byref(m), device, repeat, C.byref(host_ms), C.byref(dev_ms), mism), "wost3_mesh_build_check")
    return {k: int(mism[i]) for i, k in enumerate(MESH_BUILD_ARRAYS)}, int(mism[15]), host_ms.value, dev_ms.value


def vmf_eval(kappa, cos_theta, device=0):
    """VMF::eval(cosTheta) (reference util/vmf.h:27-32) for pairs (kappa, cos_theta)"""
    lib = capi.load()
    k = np.ascontiguousarray(kappa, dtype=np.float32)
    c = np.ascontiguousarray(cos_theta, dtype=np.float32)
    out = np.zeros(len(k), np.float32)
    _check(lib.wost3_vmf_eval(device, _fp(k), _fp(c), len(k), _fp(out)), "wost3_vmf_eval")
    return out


def vmf_sample(kappa, mu, seed, per_point=1, device=0):
    """VMF::sample(sampler, mu) (reference util/vmf.h:45-70): per point a PCG32 stream setSeed(seed, 1) and per_point
    consecutive directions about mu"""
    lib = capi.load()
    k = np.ascontiguousarray(kappa, dtype=np.float32)
    m = np.ascontiguousarray(mu, dtype=np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(seed, dtype=np.uint64)
    out = np.zeros((len(k), per_point, 3), np.float32)
    _check(lib.wost3_vmf_sample(device, _fp(k), _fp(m), s.ctypes.data_as(C.POINTER(C.c_uint64)), len(k), per_point, _fp(out)), "wost3_vmf_sample")
    return out


def vmm3_pdf_sample(raw, wi, seed, device=0, sample=True):
    """VMM<3,8>::pdf(wi) and ::sample (reference distribution.h:279-345) from 40 raw outputs per point; sample=False: the density
    alone (a null sample_dir; no stream is seeded, no direction drawn) -> (pdf, None)"""
    lib = capi.load()
    r = np.ascontiguousarray(raw, dtype=np.float32)
    w = np.ascontiguousarray(wi, dtype=np.float32).reshape(-1, 3)
    n = len(w)
    if not sample:
        pdf = np.zeros(n, np.float32)
        _check(lib.wost3_vmm_pdf_sample(device, _fp(r), _fp(w), None, n, _fp(pdf), None), "wost3_vmm_pdf_sample")
        return pdf, None
    s = np.ascontiguousarray(seed, dtype=np.uint64)
    pdf, d = np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    _check(lib.wost3_vmm_pdf_sample(device, _fp(r), _fp(w), s.ctypes.data_as(C.POINTER(C.c_uint64)), n, _fp(pdf), _fp(d)), "wost3_vmm_pdf_sample")
    return pdf, d


def vmm3_loss_gradients(raw41, dirs, li, dir_pdf, on_neumann, normal, loss_scale=128.0, device=0):
    """the loss gradient of the 3-D mixture by its 41 raw outputs (reference train.h:492-553) and the likelihood term"""
    lib = capi.load()
    r = np.ascontiguousarray(raw41, dtype=np.float32)
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    l = np.ascontiguousarray(li, dtype=np.float32)
    p = np.ascontiguousarray(dir_pdf, dtype=np.float32)
    o = np.ascontiguousarray(on_neumann, dtype=np.uint8)
    nn = np.ascontiguousarray(normal, dtype=np.float32)
    n = len(l)
    g, lk = np.zeros((n, 41), np.float32), np.zeros(n, np.float32)
    _check(lib.wost3_vmm_loss_gradients(device, _fp(r), _fp(d), _fp(l), _fp(p), o.ctypes.data_as(C.POINTER(C.c_ubyte)), _fp(nn), n,
                                        C.c_float(loss_scale), _fp(g), _fp(lk)), "wost3_vmm_loss_gradients")
    return g, lk


def default_net_config3(n_levels=8, base_resolution=8, per_level_scale=1.4049999713897705):
    """the network of GuidedIntegrator<3>: data/ladybug/n.json:49-81 with the 41 outputs of guided/parameters.h:26-33"""
    return capi.NetConfig(n_levels, 4, base_resolution, per_level_scale, 64, 3, 41, 0.00800000037997961, 0.8999999761581421,
                          0.9900000095367432, 1.0000000036274937e-15, 9.999999974752427e-07, 0.949999988079071)


class GuidedIntegrator3(GuidedCalls):
    """Mirror of GuidedIntegrator<3> (reference integrator/guided/integrator.h:77-256 with DIM = 3; exec.cu:102-122): ctor +
    resetNetwork, solve(), queryNetwork(); `aabb` = scene.aabb ((min xyz), (max xyz)); settings: GuidedIntegratorSettings"""
    _prefix, _dim, _n_out, _pos_key = "wost3_guided_", 3, 41, "xyz"      # (GuidedCalls: the solves, the training set, the network, close)

    def __init__(self, problem, settings, aabb, network_config=None, seed=42, device=0):
        self.lib = capi.load()
        self.problem, self.settings = problem, settings
        keep = []
        sc = scene3_desc(keep, problem, *settings.frameSize)
        gs = guided_settings(capi.Guided3Settings, settings)
        for k in range(3):
            gs.aabb_min[k], gs.aabb_max[k] = float(aabb[0][k]), float(aabb[1][k])
        self._open(sc, gs, network_config or default_net_config3(), seed, device)
