"""ctypes binding of the C-ABI in include/wost.h (libwost_hip.so).

This is the Python-side stub a maintainer would write against the boundary; it adds
nothing to the data path.  If the library is missing it raises -- there is no CPU
fallback in the product.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

WOST_OK = 0
MESH_DIRICHLET = 0
MESH_NEUMANN = 1


class MeshDesc(C.Structure):
    _fields_ = [
        ("n_verts", C.c_int32),
        ("n_segs", C.c_int32),
        ("verts", C.POINTER(C.c_float)),
        ("segs", C.POINTER(C.c_int32)),
        ("colors", C.POINTER(C.c_float)),
    ]


class SourceDesc(C.Structure):
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("rgb", C.POINTER(C.c_float)),
        ("index_scale", C.c_float * 2), ("index_offset", C.c_float * 2), ("intensity", C.c_float),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("dirichlet", MeshDesc),
        ("neumann", MeshDesc),
        ("dirichlet_intensity", C.c_float),
        ("neumann_intensity", C.c_float),
        ("probe_scale", C.c_float),
        ("probe_pos", C.c_float * 2),
        ("probe_up", C.c_float * 2),
        ("mask", C.POINTER(C.c_uint8)),
        ("source", SourceDesc),
    ]


class Settings(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("spp", C.c_int32),
        ("max_depth", C.c_int32),
        ("eps_shell", C.c_float),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("walk_steps", C.c_uint64),
        ("walks_started", C.c_uint64),
        ("walks_absorbed", C.c_uint64),
        ("walks_truncated", C.c_uint64),
        ("neumann_hits", C.c_uint64),
        ("inner_visits", C.c_uint64),
        ("leaf_visits", C.c_uint64),
        ("trav_trips", C.c_uint64),
        ("step_trips", C.c_uint64),
        ("solve_ms", C.c_double),
        ("kernel_ms", C.c_double),
        ("kernel_launches", C.c_uint32),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Adaptive(C.Structure):
    """wost_adaptive (include/wost.h)"""
    _fields_ = [("batch_spp", C.c_int32), ("min_batches", C.c_int32), ("max_spp", C.c_int32), ("abs_tol", C.c_float), ("rel_tol", C.c_float)]


class GradientOut(C.Structure):
    """wost_gradient_out: host pointers for the host form, device pointers for the _dev form; only grad is required"""
    _fields_ = [("grad", C.c_void_p), ("grad_stderr", C.c_void_p), ("field_rgb", C.c_void_p), ("radius", C.c_void_p),
                ("first_pts", C.c_void_p)]


class GradientCarriedOut(C.Structure):
    """wost_gradient_carried_out: host pointers for the host forms, device pointers for the _dev forms; only grad is required"""
    _fields_ = [("grad", C.c_void_p), ("grad_stderr", C.c_void_p), ("field_rgb", C.c_void_p), ("radius", C.c_void_p),
                ("batches", C.c_void_p)]


class GradientAdaptive(C.Structure):
    """wost_gradient_adaptive (include/wost.h)"""
    _fields_ = [("min_batches", C.c_int32), ("max_batches", C.c_int32), ("abs_tol", C.c_float), ("rel_tol", C.c_float)]


class ExitRecords(C.Structure):
    """wost_exit_records: host arrays of n * S entries (uv: n * S * (DIM - 1), base_rgb: n * S * 3); any may be NULL"""
    _fields_ = [("prim", C.c_void_p), ("uv", C.c_void_p), ("side", C.c_void_p), ("thp", C.c_void_p), ("base_rgb", C.c_void_p)]


class ExitGradientRecords(C.Structure):
    """wost_exit_gradient_records: host arrays of n (radius) and n * S * DIM (dirs, first_pts) floats; any may be NULL"""
    _fields_ = [("radius", C.c_void_p), ("dirs", C.c_void_p), ("first_pts", C.c_void_p)]


class Mesh3Desc(C.Structure):
    """wost3_mesh_desc (include/wost.h)"""
    _fields_ = [("n_verts", C.c_int32), ("n_tris", C.c_int32), ("verts", C.POINTER(C.c_float)), ("tris", C.POINTER(C.c_int32)),
                ("colors", C.POINTER(C.c_float))]


class Source3Desc(C.Structure):
    """wost3_source_desc (include/wost.h)"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("rgb", C.POINTER(C.c_float)),
                ("index_scale", C.c_float * 3), ("index_offset", C.c_float * 3), ("intensity", C.c_float)]


class Scene3Desc(C.Structure):
    """wost3_scene_desc (include/wost.h)"""
    _fields_ = [("dirichlet", Mesh3Desc), ("neumann", Mesh3Desc), ("dirichlet_intensity", C.c_float),
                ("neumann_intensity", C.c_float), ("probe_scale", C.c_float), ("probe_pos", C.c_float * 3),
                ("probe_up", C.c_float * 3), ("probe_right", C.c_float * 3), ("mask", C.POINTER(C.c_uint8)),
                ("source", Source3Desc)]


class NetConfig(C.Structure):
    """wost_net_config (include/wost.h); defaults = reference data/ladybug/n.json:49-81."""
    _fields_ = [
        ("n_levels", C.c_int32), ("n_features_per_level", C.c_int32), ("base_resolution", C.c_int32),
        ("per_level_scale", C.c_float),
        ("n_neurons", C.c_int32), ("n_hidden_layers", C.c_int32), ("n_output", C.c_int32),
        ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("epsilon", C.c_float),
        ("l2_reg", C.c_float), ("ema_decay", C.c_float),
    ]


class GuidedSettings(C.Structure):
    """wost_guided_settings (include/wost.h)"""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
        ("eps_shell", C.c_float), ("train_spp_count", C.c_int32),
        ("uniform_fraction_training", C.c_float), ("uniform_fraction_guiding", C.c_float),
        ("max_guided_depth_training", C.c_int32), ("max_guided_depth_guiding", C.c_int32),
        ("aabb_min", C.c_float * 2), ("aabb_max", C.c_float * 2),
        ("max_train_depth", C.c_int32), ("batch_size", C.c_int32), ("min_batch_size", C.c_int32),
        ("batches_per_spp", C.c_int32), ("train_pixel_stride", C.c_int32), ("train_pixel_offset", C.c_int32),
        ("loss_scale", C.c_float),
    ]


class Guided3Settings(C.Structure):
    """wost3_guided_settings (include/wost.h)"""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32), ("max_depth", C.c_int32),
        ("eps_shell", C.c_float), ("train_spp_count", C.c_int32),
        ("uniform_fraction_training", C.c_float), ("uniform_fraction_guiding", C.c_float),
        ("max_guided_depth_training", C.c_int32), ("max_guided_depth_guiding", C.c_int32),
        ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3),
        ("max_train_depth", C.c_int32), ("batch_size", C.c_int32), ("min_batch_size", C.c_int32),
        ("batches_per_spp", C.c_int32), ("train_pixel_stride", C.c_int32), ("train_pixel_offset", C.c_int32),
        ("loss_scale", C.c_float),
    ]


class GuidedStats(C.Structure):
    _fields_ = [
        ("walk_steps", C.c_uint64), ("walks_started", C.c_uint64), ("walks_absorbed", C.c_uint64),
        ("walks_truncated", C.c_uint64), ("neumann_hits", C.c_uint64), ("guided_steps", C.c_uint64),
        ("train_samples", C.c_uint64), ("optimizer_steps", C.c_uint64),
        ("solve_ms", C.c_double), ("train_ms", C.c_double), ("kernel_launches", C.c_uint32), ("reserved", C.c_uint32),
        ("net_points", C.c_uint64), ("net_infer_ms", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LaunchInfo(C.Structure):
    """wost_launch_info (include/wost.h)"""
    _fields_ = [("kind", C.c_int32), ("walkers", C.c_uint32), ("walkers_beside", C.c_uint32), ("grid", C.c_uint32),
                ("ms", C.c_double), ("walk_steps_done", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


LAUNCH_ROUND, LAUNCH_QUAD, LAUNCH_ONE, LAUNCH_PERSISTENT, LAUNCH_WAIT, LAUNCH_BESIDE = 0, 1, 2, 3, 4, 5
LAUNCH_NAMES = {0: "round", 1: "quad round", 2: "one launch", 3: "persistent", 4: "wait", 5: "beside only"}


# wost_sync_fn (include/wost.h): int (*)(void *user, int op, void *data, uint64_t count)
SYNC_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64)
SYNC_SUM_I64_DEVICE, SYNC_MIN_I64_HOST, SYNC_RANKS_I64_HOST = 0, 1, 2
SYNC_UNSUPPORTED = 2       # callback return value for an unknown op
# wost_frame_fn: int (*)(void *user, int reason, int32_t sample_id, double elapsed_ms, const float *field_rgb)
FRAME_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_double, C.POINTER(C.c_float))

# Every entry point of include/wost.h and its argument types, in one place: load() sets the prototypes from it and EXPORTS, the
# symbols the library must have, is its key list.  _BOTH: entries that exist as wost_<name> and wost3_<name> with one signature.
_pf, _pi, _pu8, _pu64, _pd = (C.POINTER(t) for t in (C.c_float, C.c_int32, C.c_uint8, C.c_uint64, C.c_double))
_h, _dev, _i32, _st, _gst = C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Stats), C.POINTER(GuidedStats)      # _dev: a device array or a stream
_gco = C.POINTER(GradientCarriedOut)
_pi64 = C.POINTER(C.c_int64)
_BOTH = {
    "destroy": [_h],
    "solve": [_h, _i32, _i32, _pf, _st],
    "solve_sharded": [_h, _i32, _i32, _dev, _dev, _st],
    "solve_points": [_h, _pf, _i32, _i32, _i32, _pf, _st],
    "solve_points_dev": [_h, _dev, _i32, _i32, _i32, _dev, _dev, _st],
    # the carried frame solve (wost_solve_more & co.)
    "solve_more": [_h, _i32, _pf, _st],
    "solve_more_sharded": [_h, _i32, _i32, _i32, _dev, _dev, _st],
    "solve_restart": [_h],
    "solve_progress": [_h, _pi],
    "solve_more_where": [_h, _i32, _pu8, _pf, _st],
    "solve_more_where_sharded": [_h, _i32, _i32, _i32, _dev, _dev, _dev, _st],
    "solve_carried": [_h, _pi, _pi, _pf, _pf],
    "solve_adaptive": [_h, C.POINTER(Adaptive), _pf, _pf, _pi, _st],
    "solve_adaptive_sharded": [_h, _i32, _i32, C.POINTER(Adaptive), _dev, _dev, _st],
    # the carried point list (wost_points_carry & co.)
    "points_carry": [_h, _pf, _i32, _i32, _i32],
    "points_carry_dev": [_h, _dev, _i32, _i32, _i32, _dev],
    "points_more": [_h, _i32, _pu8, _pf, _st],
    "points_more_dev": [_h, _i32, _dev, _dev, _dev, _st],
    "points_carried": [_h, _pi, _pi, _pf, _pf],
    "points_adaptive": [_h, C.POINTER(Adaptive), _pf, _pf, _pi, _st],
    "points_adaptive_dev": [_h, C.POINTER(Adaptive), _dev, _dev, _st],
    "points_restart": [_h],
    "points_progress": [_h, _pi, _pi],
    # the gradient at the caller's points (wost_solve_gradient_points & co.)
    "solve_gradient_points": [_h, _pf, _i32, _i32, _i32, _i32, C.POINTER(GradientOut), _st],
    "solve_gradient_points_dev": [_h, _dev, _i32, _i32, _i32, _i32, C.POINTER(GradientOut), _dev, _st],
    # the carried gradient list (wost_gradient_points_carry & co.)
    "gradient_points_carry": [_h, _pf, _i32, _i32, _i32, _i32, _i32, _i32, _i32],
    "gradient_points_carry_dev": [_h, _dev, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _dev],
    "gradient_points_more": [_h, _pu8, _gco, _st],
    "gradient_points_more_dev": [_h, _dev, _gco, _dev, _st],
    "gradient_points_carried": [_h, _gco],
    "gradient_points_adaptive": [_h, C.POINTER(GradientAdaptive), _gco, _st],
    "gradient_points_adaptive_dev": [_h, C.POINTER(GradientAdaptive), _gco, _dev, _st],
    "gradient_points_restart": [_h],
    "gradient_points_progress": [_h, _pi, _pi],
    # the exit list (wost_exits_walk & co.)
    "exits_walk": [_h, _pf, _i32, _i32, _i32, _i32, _st],
    "exits_walk_dev": [_h, _dev, _i32, _i32, _i32, _i32, _dev, _st],
    "exits_records": [_h, C.POINTER(ExitRecords)],
    "exits_apply": [_h, _pf, _i32, _pf, _pf],
    "exits_apply_dev": [_h, _dev, _i32, _dev, _dev, _dev],
    "exits_adjoint": [_h, _pf, _i32, _pf],
    "exits_adjoint_dev": [_h, _dev, _i32, _dev, _dev],
    "exits_progress": [_h, _pi, _pi],
    # the exit list of the gradient (wost_exits_walk_gradient & co.)
    "exits_walk_gradient": [_h, _pf, _i32, _i32, _i32, _i32, _i32, _st],
    "exits_walk_gradient_dev": [_h, _dev, _i32, _i32, _i32, _i32, _i32, _dev, _st],
    "exits_gradient_records": [_h, C.POINTER(ExitGradientRecords)],
    "exits_apply_gradient": [_h, _pf, _i32, _pf, _pf, _pf],
    "exits_apply_gradient_dev": [_h, _dev, _i32, _dev, _dev, _dev, _dev],
    "exits_gradient_terms": [_h, _pd, _pd, _pd],
    "exits_adjoint_gradient": [_h, _pf, _i32, _pf],
    "exits_adjoint_gradient_dev": [_h, _dev, _i32, _dev, _dev],
    # the index of the exit list and the ordered adjoints (wost_exits_index & co.)
    "exits_index": [_h],
    "exits_index_info": [_h, _pi64, _pi64],
    "exits_index_records": [_h, _pi64, _pi],
    "exits_adjoint_ordered": [_h, _pf, _i32, _pf],
    "exits_adjoint_ordered_dev": [_h, _dev, _i32, _dev, _dev],
    "exits_adjoint_gradient_ordered": [_h, _pf, _i32, _pf],
    "exits_adjoint_gradient_ordered_dev": [_h, _dev, _i32, _dev, _dev],
    # the batch queries
    "render_sdf": [_h, C.c_int, _pf],
    "render_source": [_h, _pf],
    "closest_point": [_h, C.c_int, _pf, _i32, _pi, _pf, _pf, _pi],
    "closest_silhouette": [_h, C.c_int, _pf, _pf, _i32, _pf],
    "ray_intersect": [_h, C.c_int, _pf, _pf, _pf, _i32, _pi, _pf, _pi],
    # the mixture, the network and the guided solves
    "vmm_pdf_sample": [C.c_int, _pf, _pf, _pu64, _i32, _pf, _pf],
    "vmm_loss_gradients": [C.c_int, _pf, _pf, _pf, _pf, _pu8, _pf, _i32, C.c_float, _pf, _pf],
    "net_create": [C.c_int, C.POINTER(NetConfig), C.c_uint64, C.POINTER(_h)],
    "guided_destroy": [_h],
    "guided_network": [_h, C.POINTER(_h)],
    "guided_scene": [_h, C.POINTER(_h)],
    "guided_query_network": [_h, _pf, _i32, _pf],
    "guided_solve": [_h, _pf, _gst],
    "guided_solve_sharded": [_h, _i32, _i32, _dev, _gst],
    "guided_solve_points": [_h, _pf, _i32, _i32, _i32, _i32, _pf, _gst],
    "guided_solve_points_dev": [_h, _dev, _i32, _i32, _i32, _i32, _dev, _gst],
    "guided_train_set": [_h, _i32, _pi, _pf, _pf, _pf, _pf, _pf, _pu8],
}
SIGNATURES = {pre + name: sig for pre in ("wost_", "wost3_") for name, sig in _BOTH.items()}
SIGNATURES.update({
    "wost_last_error": [], "wost_version": [],
    "wost_create": [C.POINTER(SceneDesc), C.POINTER(Settings), C.c_int, C.POINTER(_h)],
    "wost3_create": [C.POINTER(Scene3Desc), C.POINTER(Settings), C.c_int, C.POINTER(_h)],
    "wost_mesh_build_check": [C.POINTER(MeshDesc), C.c_int, _i32, _pd, _pd, C.POINTER(C.c_int64)],
    "wost3_mesh_build_check": [C.POINTER(Mesh3Desc), C.c_int, _i32, _pd, _pd, C.POINTER(C.c_int64)],
    "wost_guided_create": [C.POINTER(SceneDesc), C.POINTER(GuidedSettings), C.POINTER(NetConfig), C.c_uint64, C.c_int, C.POINTER(_h)],
    "wost3_guided_create": [C.POINTER(Scene3Desc), C.POINTER(Guided3Settings), C.POINTER(NetConfig), C.c_uint64, C.c_int, C.POINTER(_h)],
    # 2-D alone
    "wost_set_option": [_h, C.c_char_p, C.c_double],
    "wost_last_launches": [_h, C.POINTER(LaunchInfo), _i32, _pi],
    "wost_vonmises_eval": [C.c_int, _pf, _pf, _i32, _pf, _pf, _pf, _pf],
    "wost_vonmises_sample": [C.c_int, _pf, _pu64, _i32, _i32, _pf],
    "wost_net_destroy": [_h],
    "wost_net_n_params": [_h, _pu64, _pu64],
    "wost_net_get_params": [_h, C.c_int, _pf],
    "wost_net_set_params": [_h, _pf],
    "wost_net_set_gradient_buffer": [_h, _dev],
    "wost_net_inference": [_h, _pf, _i32, _pf, C.c_int],
    "wost_net_train_step": [_h, _pf, _pf, _i32, C.c_float, C.c_int],
    "wost_net_set_option": [_h, C.c_char_p, C.c_double],
    "wost_guided_set_sync": [_h, SYNC_FN, _h],
    "wost_guided_set_frame_callback": [_h, FRAME_FN, _h, _i32, _i32, _i32],
    "wost_guided_set_option": [_h, C.c_char_p, C.c_double],
    # 3-D alone
    "wost3_set_option": [_h, C.c_char_p, C.c_double],
    "wost3_vmf_eval": [C.c_int, _pf, _pf, _i32, _pf],
    "wost3_vmf_sample": [C.c_int, _pf, _pf, _pu64, _i32, _i32, _pf],
})
EXPORTS = list(SIGNATURES)

_lib = None


def library_path():
    # WOST_LIB: developer override to A/B alternative builds of the same C-ABI
    return os.environ.get("WOST_LIB", _build.LIB_PATH)


def load():
    """Load libwost_hip.so (built in-tree by elaina_amd.build). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; loading it FIRST makes this library bind to the same
    # HIP runtime (same SONAME), so one process never holds two runtimes (DESIGN.md "runtime").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "libwost_hip.so is missing (%s): run `python -m elaina_amd.build`; "
            "this package has no CPU fallback" % path)
    L = C.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        getattr(L, name).argtypes = argtypes  # (fails loudly on a missing symbol)
    L.wost_last_error.restype = C.c_char_p
    L.wost_version.restype = C.c_char_p
    _lib = L
    return L


class WostError(RuntimeError):
    pass


def _check(rc, what):
    if rc != WOST_OK:
        raise WostError("%s failed (%d): %s" % (what, rc, load().wost_last_error().decode()))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))
