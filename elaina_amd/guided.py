"""Python stub for the guided path's distribution layer of the C-ABI (include/wost.h):
von Mises log-Bessel / pdf / d-dkappa, rejection sampling, and the 8-lobe mixture VMM<2,8>.
Thin ctypes calls; no arithmetic here."""
import ctypes as C

import numpy as np

from . import capi
from .capi import _check, _fp


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def vonmises_eval(kappa, cos_theta, device=0):
    lib = capi.load()
    k = np.ascontiguousarray(kappa, dtype=np.float32)
    c = np.ascontiguousarray(cos_theta, dtype=np.float32)
    n = len(k)
    out = [np.zeros(n, dtype=np.float32) for _ in range(4)]
    _check(lib.wost_vonmises_eval(device, _fp(k), _fp(c), n, *[_fp(o) for o in out]), "wost_vonmises_eval")
    return dict(zip(("log_i0", "log_i1", "log_pdf", "dlog_dkappa"), out))


def vonmises_sample(kappa, seed, per_point=1, device=0):
    lib = capi.load()
    k = np.ascontiguousarray(kappa, dtype=np.float32)
    s = np.ascontiguousarray(seed, dtype=np.uint64)
    th = np.zeros(len(k) * per_point, dtype=np.float32)
    _check(lib.wost_vonmises_sample(device, _fp(k), _u64(s), len(k), per_point, _fp(th)), "wost_vonmises_sample")
    return th.reshape(len(k), per_point)


def vmm_pdf_sample(raw, wi, seed, device=0, sample=True):
    """sample=False: the density alone (a null sample_dir; no stream is seeded, no direction drawn) -> (pdf, None)"""
    lib = capi.load()
    r = np.ascontiguousarray(raw, dtype=np.float32)
    w = np.ascontiguousarray(wi, dtype=np.float32)
    n = len(w)
    pdf = np.zeros(n, dtype=np.float32)
    if not sample:
        _check(lib.wost_vmm_pdf_sample(device, _fp(r), _fp(w), None, n, _fp(pdf), None), "wost_vmm_pdf_sample")
        return pdf, None
    s = np.ascontiguousarray(seed, dtype=np.uint64)
    d = np.zeros((n, 2), dtype=np.float32)
    _check(lib.wost_vmm_pdf_sample(device, _fp(r), _fp(w), _u64(s), n, _fp(pdf), _fp(d)), "wost_vmm_pdf_sample")
    return pdf, d


def vmm_loss_gradients(raw33, dirs, li, dir_pdf, on_neumann, normal, loss_scale=128.0, device=0):
    lib = capi.load()
    r = np.ascontiguousarray(raw33, dtype=np.float32)
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    l = np.ascontiguousarray(li, dtype=np.float32)
    p = np.ascontiguousarray(dir_pdf, dtype=np.float32)
    o = np.ascontiguousarray(on_neumann, dtype=np.uint8)
    nn = np.ascontiguousarray(normal, dtype=np.float32)
    n = len(l)
    g = np.zeros((n, 33), dtype=np.float32)
    lk = np.zeros(n, dtype=np.float32)
    _check(lib.wost_vmm_loss_gradients(device, _fp(r), _fp(d), _fp(l), _fp(p), o.ctypes.data_as(C.POINTER(C.c_uint8)),
                                       _fp(nn), n, C.c_float(loss_scale), _fp(g), _fp(lk)), "wost_vmm_loss_gradients")
    return g, lk


def default_net_config():
    """Network of the reference's 2-D guided integrator: data/ladybug/n.json:49-81, 33 outputs
    (8 lobes x (kappa, mu.x, mu.y, weight) + selection logit, guided/parameters.h:16-24)."""
    return capi.NetConfig(8, 4, 8, 1.4049999713897705, 64, 3, 33, 0.00800000037997961, 0.8999999761581421,
                          0.9900000095367432, 1.0000000036274937e-15, 9.999999974752427e-07, 0.949999988079071)


class GuidingNetwork:
    """Device-resident guiding network (wost_net_* of include/wost.h): DenseGrid encoding ->
    ReLU MLP, Adam nested in EMA.  Mirrors how integrator/guided/integrator.cu drives
    tiny-cuda-nn: inference() (:560,:597) and one training step (:655-662)."""

    def __init__(self, config=None, seed=1337, device=0, dims=2):
        """dims = 3: the three-input network of GuidedIntegrator<3> (wost3_net_create)"""
        self._lib = capi.load()
        self.config = config or default_net_config()
        self.dims = dims
        self._h = C.c_void_p()
        create = self._lib.wost3_net_create if dims == 3 else self._lib.wost_net_create
        _check(create(device, C.byref(self.config), seed, C.byref(self._h)), "wost_net_create")
        total, mlp = C.c_uint64(), C.c_uint64()
        _check(self._lib.wost_net_n_params(self._h, C.byref(total), C.byref(mlp)), "wost_net_n_params")
        self.n_params, self.n_mlp_params = total.value, mlp.value

    def close(self):
        if self._h:
            self._lib.wost_net_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _get(self, which):
        out = np.zeros(self.n_params, dtype=np.float32)
        _check(self._lib.wost_net_get_params(self._h, which, _fp(out)), "wost_net_get_params")
        return out

    def params(self):
        return self._get(0)

    def inference_params(self):
        return self._get(1)

    def gradients(self):
        return self._get(2)

    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=np.float32)
        if p.size != self.n_params:
            raise ValueError("expected %d parameters" % self.n_params)
        _check(self._lib.wost_net_set_params(self._h, _fp(p)), "wost_net_set_params")

    def set_option(self, key, value):
        """"precision": 32 (fp32, bit-exact mode, default) or 16 (the reference's half-precision inference);
        "train_precision": 32 (default) or 16 (forward / backward / weight gradients of the training steps on
        f16 matrix instructions, fp32 master weights)"""
        _check(self._lib.wost_net_set_option(self._h, key.encode(), float(value)), "wost_net_set_option")

    def inference(self, xy, use_inference_params=True):
        x = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, getattr(self, "dims", 2))
        out = np.zeros((len(x), self.config.n_output), dtype=np.float32)
        _check(self._lib.wost_net_inference(self._h, _fp(x), len(x), _fp(out), int(use_inference_params)),
               "wost_net_inference")
        return out

    def train_step(self, xy, dl_dout, loss_scale=128.0, apply_update=True):
        x = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, getattr(self, "dims", 2))
        g = np.ascontiguousarray(dl_dout, dtype=np.float32).reshape(len(x), self.config.n_output)
        _check(self._lib.wost_net_train_step(self._h, _fp(x), _fp(g), len(x), loss_scale, int(apply_update)),
               "wost_net_train_step")


class GuidedIntegratorSettings:
    """reference integrator/guided/integrator.h:54-75; the trailing group exposes the reference's
    compile-time training constants (parameters.h:7-14, integrator.h:237-239)"""

    def __init__(self, frameSize=(800, 800), samplesPerPixel=512, trainSppCount=150,
                 uniformFractionInTrainingPhase=0.5, uniformFractionInGuidingPhase=0.5,
                 maxGuidedDepthInTrainingPhase=10, maxGuidedDepthInGuidingPhase=10, maxWalkingDepth=32,
                 epsilonShell=1e-5, debugPixel=0, saveSppMetricsDuration=-1, saveSppMetricsUntil=1024,
                 saveTimeMetricsDuration=-1,
                 maxTrainDepth=3, batchSize=524288, minBatchSize=65536, batchPerFrame=5, trainPixelStride=1,
                 trainPixelOffset=-1, lossScale=128.0):
        self.frameSize = (int(frameSize[0]), int(frameSize[1]))
        self.samplesPerPixel = int(samplesPerPixel)
        self.trainSppCount = int(trainSppCount)
        self.uniformFractionInTrainingPhase = float(uniformFractionInTrainingPhase)
        self.uniformFractionInGuidingPhase = float(uniformFractionInGuidingPhase)
        self.maxGuidedDepthInTrainingPhase = int(maxGuidedDepthInTrainingPhase)
        self.maxGuidedDepthInGuidingPhase = int(maxGuidedDepthInGuidingPhase)
        self.maxWalkingDepth = int(maxWalkingDepth)
        self.epsilonShell = float(epsilonShell)
        self.debugPixel = debugPixel
        self.saveSppMetricsDuration = saveSppMetricsDuration
        self.saveSppMetricsUntil = saveSppMetricsUntil
        self.saveTimeMetricsDuration = saveTimeMetricsDuration
        self.maxTrainDepth, self.batchSize, self.minBatchSize = int(maxTrainDepth), int(batchSize), int(minBatchSize)
        self.batchPerFrame, self.trainPixelStride, self.trainPixelOffset = int(batchPerFrame), int(trainPixelStride), int(trainPixelOffset)
        self.lossScale = float(lossScale)


class _BorrowedNetwork(GuidingNetwork):
    """the integrator's own network: same methods, lifetime owned by the integrator"""

    def __init__(self, lib, handle, config, dims=2):
        self._lib, self._h, self.config, self.dims = lib, handle, config, dims
        total, mlp = C.c_uint64(), C.c_uint64()
        _check(lib.wost_net_n_params(handle, C.byref(total), C.byref(mlp)), "wost_net_n_params")
        self.n_params, self.n_mlp_params = total.value, mlp.value

    def close(self):
        self._h = C.c_void_p()


def guided_settings(struct, settings):
    """a capi.GuidedSettings or capi.Guided3Settings with every field the two have in common filled in (the box is the caller's)"""
    w, h = settings.frameSize
    gs = struct(w, h, settings.samplesPerPixel, settings.maxWalkingDepth, settings.epsilonShell, settings.trainSppCount,
                settings.uniformFractionInTrainingPhase, settings.uniformFractionInGuidingPhase, settings.maxGuidedDepthInTrainingPhase,
                settings.maxGuidedDepthInGuidingPhase)
    gs.max_train_depth, gs.batch_size, gs.min_batch_size = settings.maxTrainDepth, settings.batchSize, settings.minBatchSize
    gs.batches_per_spp, gs.train_pixel_stride = settings.batchPerFrame, settings.trainPixelStride
    gs.train_pixel_offset, gs.loss_scale = settings.trainPixelOffset, settings.lossScale
    return gs


class GuidedCalls:
    """What GuidedIntegrator and GuidedIntegrator3 have in common: every method whose entry points exist as wost_guided_* and
    wost3_guided_* (include/wost.h) with the same arguments.  Base of an integrator with .lib, ._handle, .n_pixels, .settings,
    .network, ._prefix ("wost_guided_" or "wost3_guided_"), ._dim (2 or 3), ._n_out (raw network outputs per point) and ._pos_key
    (the training set's position key)."""

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name), self._prefix + name

    def _open(self, scene, gs, network_config, seed, device):
        """the handle of a new integrator and its network, borrowed"""
        self.network_config = network_config
        self._handle = C.c_void_p()
        fn, name = self._fn("create")
        _check(fn(C.byref(scene), C.byref(gs), C.byref(network_config), seed, device, C.byref(self._handle)), name)
        nh = C.c_void_p()
        fn, name = self._fn("network")
        _check(fn(self._handle, C.byref(nh)), name)
        self.network = _BorrowedNetwork(self.lib, nh, network_config, dims=self._dim)
        self.n_pixels = self.settings.frameSize[0] * self.settings.frameSize[1]
        self.solution, self.last_stats = None, None

    def _solve(self, entry, *args):
        """an entry point whose last argument is the stats -> the stats"""
        fn, name = self._fn(entry)
        st = capi.GuidedStats()
        _check(fn(self._handle, *args, C.byref(st)), name)
        self.last_stats = st.as_dict()
        return st

    def _point_seeds(self, seed_base, seed_width, train_spp):
        width = self.settings.frameSize[0] if seed_width is None else seed_width
        return int(seed_base), int(width), -1 if train_spp is None else int(train_spp)

    def close(self):
        if self._handle:
            self.network.close()
            self._fn("destroy")[0](self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self):
        """returns wall milliseconds like the reference; the field is in self.solution"""
        field = np.zeros((self.n_pixels, 3), dtype=np.float32)
        st = self._solve("solve", _fp(field))
        self.solution = field
        return int(st.solve_ms)

    def solve_sharded(self, shard_index, shard_count, field_dev_ptr):
        """field_dev_ptr: device pointer (int) to a width*height*3 float buffer; returns the stats"""
        self._solve("solve_sharded", shard_index, shard_count, C.c_void_p(field_dev_ptr))
        return self.last_stats

    def solve_points(self, points, seed_base=0, seed_width=None, train_spp=None):
        """the guided solve at the caller's evaluation points ([n, dim] floats, at most frame width * height of them) instead of the
        frame's pixels (wost_guided_solve_points, wost3_guided_solve_points): point i takes the place of pixel i of a solve over n
        pixels, on the random stream of pixel seed_base + i in a frame seed_width wide (default: the frame's width).  train_spp:
        None = the settings' trainSppCount, otherwise the number of training samples of this call -- 0 probes with the network as
        it is and leaves it unchanged.  Returns the (n, 3) float32 field; the counters are in last_stats"""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, self._dim)
        field = np.zeros((len(p), 3), dtype=np.float32)
        self._solve("solve_points", _fp(p), len(p), *self._point_seeds(seed_base, seed_width, train_spp), _fp(field))
        return field

    def solve_points_dev(self, points_ptr, n, field_ptr, seed_base=0, seed_width=None, train_spp=None):
        """the same on device pointers (ints): n * dim floats of points, complete when the call is made, and n * 3 floats of field;
        runs on the integrator's own stream and returns the stats when the work is complete.  A point with a non-finite coordinate
        is not walked: its field entry is NaN"""
        self._solve("solve_points_dev", C.c_void_p(points_ptr), int(n), *self._point_seeds(seed_base, seed_width, train_spp), C.c_void_p(field_ptr))
        return self.last_stats

    def train_set(self):
        """training set of the most recent training pass, (pixel, record) order"""
        fn, name = self._fn("train_set")
        n = C.c_int32()
        _check(fn(self._handle, 0, C.byref(n), None, None, None, None, None, None), name)
        m, d = n.value, self._dim
        out = {self._pos_key: np.zeros((m, d), np.float32), "dir": np.zeros((m, d), np.float32),
               "solution": np.zeros((m, 3), np.float32), "dir_pdf": np.zeros(m, np.float32),
               "normal": np.zeros((m, d), np.float32), "on_neumann": np.zeros(m, np.uint8)}
        if m:
            _check(fn(self._handle, m, C.byref(n), _fp(out[self._pos_key]), _fp(out["dir"]), _fp(out["solution"]), _fp(out["dir_pdf"]),
                      _fp(out["normal"]), out["on_neumann"].ctypes.data_as(C.POINTER(C.c_uint8))), name)
        return out

    def queryNetwork(self, p):
        """raw mixture parameters of the guiding network at world position(s) p (reference
        integrator.cu:566-615 prints the VMM built from them)"""
        fn, name = self._fn("query_network")
        pts = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, self._dim)
        raw = np.zeros((len(pts), self._n_out), dtype=np.float32)
        _check(fn(self._handle, _fp(pts), len(pts), _fp(raw)), name)
        return raw if np.ndim(p) > 1 else raw[0]


class GuidedIntegrator(GuidedCalls):
    """Mirror of GuidedIntegrator<2> (reference integrator/guided/integrator.h:77-256): ctor +
    resetNetwork, solve(), queryNetwork(); `aabb` is scene.aabb of the JSON configuration."""
    _prefix, _dim, _n_out, _pos_key = "wost_guided_", 2, 33, "xy"      # (GuidedCalls: the solves, the training set, the network, close)

    def __init__(self, problem, settings, aabb, network_config=None, seed=42, device=0):
        from .integrator import scene_desc
        self.lib = capi.load()
        self.problem, self.settings = problem, settings
        keep = []
        sc = scene_desc(keep, problem, *settings.frameSize)
        gs = guided_settings(capi.GuidedSettings, settings)
        (gs.aabb_min[0], gs.aabb_min[1]), (gs.aabb_max[0], gs.aabb_max[1]) = aabb
        self._open(sc, gs, network_config or default_net_config(), seed, device)
        self.aabb = aabb

    def set_option(self, key, value):
        """wost_guided_set_option: "pipeline" 1 = the pipelined training order (sample k + 1 walks with the weights of training
        pass k - 1 while pass k trains on a second stream; statistically equivalent, never the parity mode)"""
        _check(self.lib.wost_guided_set_option(self._handle, key.encode(), float(value)), "wost_guided_set_option")

    def share_network(self):
        """Train ONE network across all ranks of the initialised torch.distributed group
        (wost_guided_set_sync): the fixed-point gradient buffer lives in a torch tensor, which is
        all-reduced (RCCL over xGMI with the nccl backend) before every Adam step; integer sums
        keep the ranks' networks bit-identical.  Without this call every shard trains its own."""
        import torch
        import torch.distributed as dist
        self._grad = torch.zeros(self.network.n_params, dtype=torch.int64, device="cuda")
        _check(self.lib.wost_net_set_gradient_buffer(self.network._h, C.c_void_p(self._grad.data_ptr())),
               "wost_net_set_gradient_buffer")

        from . import distributed as D
        body = D.make_network_sync(self._grad, torch.cuda.synchronize)

        def sync(user, op, data, count):
            return body(op, data, count)

        self._sync = capi.SYNC_FN(sync)       # keep the trampoline alive
        _check(self.lib.wost_guided_set_sync(self._handle, self._sync, None), "wost_guided_set_sync")
