"""The guiding network away from the reference's shape and outside the unit square.

wost_net_create accepts a family of shapes (1-16 levels x 1-8 features, encoded width <= 64 and a multiple of 8; 8-64 neurons, a multiple of
8; 1-15 hidden layers; 1-64 outputs; any base resolution >= 1 and per-level scale >= 1).  Everything but 32 -> 3 x 64 -> 48 runs on the
one-thread-per-point kernels with a gradient plan of its own (make_train_plan); the shapes below reach the branches of that code which the
reference shape never takes.  CPU part: the oracle (oracle/wost_net.c) against a float64 numpy restatement at every shape, so that it is a
checked reference there, and the refusal of every shape just outside the family.  GPU part: the HIP network against the oracle bit for bit
at these shapes; inputs outside [0, 1]^2 (the 32-bit index rule of DESIGN.md 4.7); guided solves with the guiding box inside the domain,
and one on a network of another shape."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import NetConfig, Oracle, default_net_config
from test_guided_3d import _hip_cfg
from test_guided_integrator import _gpu_and_oracle, laplace_box
from test_guided_network import _half_network_numpy, _rand_params

WOST_ERR_UNSUPPORTED = -3

# id -> (levels, features, base resolution, per-level scale, neurons, hidden layers, outputs) and what the shape reaches
SHAPES2 = {
    "mfma_16x2": (16, 2, 4, 1.2, 64, 3, 33),     # MFMA forward NF = 0; one-launch plan of 6 groups
    "mfma_4x8": (4, 8, 8, 1.405, 64, 3, 33),     # MFMA NF = 0 with 8 features; plan of 3 groups, replicas 4 / 4 / 2
    "mfma_out48": (8, 4, 8, 1.405, 64, 3, 48),   # MFMA kernels with no padded output row ...
    "mfma_out34": (8, 4, 8, 1.405, 64, 3, 34),   # ... and with 14
    "tiny": (2, 4, 1, 1.0, 8, 1, 1),             # every minimum at once: levels of one cell, scale 1, one output padded to 16, 8 replicas
    "wide": (8, 8, 2, 2.0, 64, 2, 64),           # enc 64 and 64 outputs; plan cleared (> 16 groups); fallback of 13 steps, last level use_lds = 0
    "deep": (16, 4, 3, 1.3, 24, 15, 5),          # 15 hidden layers of width 24; 16 levels; fallback with slices and use_lds = 0
    "big_grid": (8, 1, 8, 2.0, 32, 2, 17),       # one feature per level, 1.4 M grid floats, three levels through global atomics
    "sliced": (4, 2, 16, 1.7, 16, 1, 16),        # enc 8; one-launch plan whose finest level is cut into one-feature slices
}
SHAPES3 = {"tiny": SHAPES2["tiny"], "small": (4, 2, 4, 1.5, 16, 2, 41)}
CASES = [(2, k) for k in SHAPES2] + [(3, k) for k in SHAPES3]
CASE_IDS = ["%dd-%s" % c for c in CASES]


@pytest.fixture(scope="module")
def orc():
    return Oracle()


def _cfg(shape):
    """the oracle's NetConfig of a shape (outputs padded to 16 like the library's), optimizer constants of the reference configuration"""
    d = default_net_config()
    nl, nf, base, scale, neurons, hidden, n_out = shape
    return NetConfig(nl, nf, base, scale, neurons, hidden, n_out, (n_out + 15) // 16 * 16, d.learning_rate, d.beta1, d.beta2, d.epsilon,
                     d.l2_reg, d.ema_decay)


def _case(dims, key):
    return _cfg((SHAPES3 if dims == 3 else SHAPES2)[key])


def _params(orc, cfg, seed, dims=2, gscale=0.5):
    """_rand_params with matrices wide enough (He-uniform) that 15 ReLU layers of width 24 still pass a signal"""
    return _rand_params(orc, cfg, seed=seed, wscale=float(np.sqrt(6.0 / cfg.n_neurons)), gscale=gscale, dims=dims)


def _n_mlp(cfg):
    return cfg.n_neurons * (cfg.n_levels * cfg.n_features + (cfg.n_hidden_layers - 1) * cfg.n_neurons + cfg.n_output_padded)


def _forward(orc, cfg, dims, p, x):
    return orc.net3_forward(cfg, p, x) if dims == 3 else orc.net_forward(cfg, p, x)[0]


def _backward(orc, cfg, dims, p, x, dl):
    dlp = np.zeros((len(x), cfg.n_output_padded), np.float32)
    dlp[:, :cfg.n_output] = dl
    return (orc.net3_backward if dims == 3 else orc.net_backward)(cfg, p, x, dlp)


def _opt_state(n):
    st = {k: np.zeros(n, np.float32) for k in ("m1", "m2", "ema_raw")}
    st["steps"] = np.zeros(n, np.uint32)
    return st


def _opt_step(orc, cfg, dims, p, st, g, step):
    return (orc.net3_optimizer_step if dims == 3 else orc.net_optimizer_step)(cfg, p, st, g, step, 128.0)


FAR = np.array([[-3.7, 2.5], [2.5, -3.7], [1.0e6, -1.0e6], [-1.0e6, 0.3]], np.float32)


def _points(rng, n, dims, lo=0.0, hi=1.0, far=False):
    x = rng.uniform(lo, hi, (n, dims)).astype(np.float32)
    if n >= 2:
        x[0, :2], x[1, :2] = (0.0, 1.0), (1.0, 1.0)          # corners of the square: the last cell, weight exactly 0 or 1
    if far and n >= 2 + len(FAR):
        x[2:2 + len(FAR), :2] = FAR
    return x


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------
def _levels64(orc, cfg, dims):
    """grid_scale = base * s^level - 1, grid_resolution = ceil(scale) + 1, res^dims entries rounded up to 8 -- in float64, checked against
    the oracle's fp32 numbers (wo_net_levels); the fp32 scales are the ones the positions are formed with"""
    res, scale, enc = orc.net_levels(cfg)
    s64 = np.exp2(np.arange(cfg.n_levels) * np.log2(float(np.float32(cfg.per_level_scale)))) * cfg.base_resolution - 1.0
    np.testing.assert_allclose(scale, s64, rtol=2e-6, atol=1e-6)
    assert [int(r) for r in res] == [int(np.ceil(float(s))) + 1 for s in scale] and enc == cfg.n_levels * cfg.n_features
    n_level = [(int(r) ** dims + 7) // 8 * 8 for r in res]
    return [int(r) for r in res], [float(s) for s in scale], n_level


def _encode64(cfg, dims, res, scale, n_level, x):
    """-> per level the entry index [n, 2^dims] and the weight [n, 2^dims] of every corner.  The position is the one fp32 fma of both
    sides, pos = fl32(scale * x + 0.5) -- it decides the cell, so it belongs to the index rule -- and everything after it is float64.
    Index rule: cell = floor(pos) as int, reinterpreted as uint32; two inputs: (cx + cy * res) mod 2^32, three inputs:
    cx + cy * res + cz * res^2 in 64 bits; then mod the level's padded entry count."""
    idx, wgt = [], []
    for lv in range(cfg.n_levels):
        pos = (np.float64(np.float32(scale[lv])) * x.astype(np.float64) + 0.5).astype(np.float32).astype(np.float64)
        fl = np.floor(pos)
        frac = pos - fl
        cell = fl.astype(np.int64)
        I = np.zeros((len(x), 1 << dims), np.int64)
        W = np.ones((len(x), 1 << dims))
        for k in range(1 << dims):
            c = [(cell[:, d] + ((k >> d) & 1)) % (1 << 32) for d in range(dims)]
            for d in range(dims):
                W[:, k] *= frac[:, d] if (k >> d) & 1 else 1.0 - frac[:, d]
            lin = (c[0] + c[1] * res[lv]) % (1 << 32) if dims == 2 else c[0] + c[1] * res[lv] + c[2] * res[lv] * res[lv]
            I[:, k] = lin % n_level[lv]
        idx.append(I)
        wgt.append(W)
    return idx, wgt


def _net64(cfg, dims, levels, p, x, dl):
    """encoding, bias-free ReLU MLP and, by the chain rule, d<dl, out>/d(parameters): all float64.  -> out, enc, gradient (parameter order)"""
    res, scale, n_level = levels
    nf, E, H, NL, NO = cfg.n_features, cfg.n_levels * cfg.n_features, cfg.n_neurons, cfg.n_hidden_layers, cfg.n_output_padded
    p64 = p.astype(np.float64)
    shapes = [(H, E)] + [(H, H)] * (NL - 1) + [(NO, H)]
    Ws, off = [], 0
    for no, ni in shapes:
        Ws.append(p64[off:off + no * ni].reshape(no, ni))
        off += no * ni
    grids = []
    for lv in range(cfg.n_levels):
        grids.append(p64[off:off + n_level[lv] * nf].reshape(n_level[lv], nf))
        off += n_level[lv] * nf
    assert off == len(p)
    idx, wgt = _encode64(cfg, dims, res, scale, n_level, x)
    enc = np.concatenate([np.einsum("nk,nkf->nf", wgt[lv], grids[lv][idx[lv]]) for lv in range(cfg.n_levels)], axis=1)
    acts = [enc]
    for W in Ws[:-1]:
        acts.append(np.maximum(acts[-1] @ W.T, 0.0))
    out = acts[-1] @ Ws[-1].T
    d = np.zeros((len(x), NO))
    d[:, :cfg.n_output] = dl
    gW = [None] * len(Ws)
    for layer in range(NL, -1, -1):
        gW[layer] = d.T @ acts[layer]
        d = d @ Ws[layer]
        if layer > 0:
            d = np.where(acts[layer] > 0, d, 0.0)
    gG = []
    for lv in range(cfg.n_levels):
        g = np.zeros_like(grids[lv])
        denc = d[:, lv * nf:(lv + 1) * nf]
        for k in range(1 << dims):
            np.add.at(g, idx[lv][:, k], wgt[lv][:, k, None] * denc)
        gG.append(g)
    return out, enc, np.concatenate([g.ravel() for g in gW + gG]), [w.size for w in Ws], [g.size for g in gG]


# Worst deviation oracle <-> float64 restatement, as a fraction of the largest reference magnitude of the compared array (70 points, the
# seeds below), measured when this test was written -- forward / encoding / matrix gradients / grid gradients:
#   2d-mfma_16x2 2.6e-7 1.0e-7 2.6e-7 3.9e-7     2d-mfma_4x8 2.0e-7 1.0e-7 2.3e-7 3.2e-7     2d-mfma_out48 1.8e-7 8.7e-8 2.1e-7 3.7e-7
#   2d-mfma_out34 1.8e-7 8.7e-8 4.0e-7 3.4e-7    2d-tiny 8.6e-8 2.5e-8 6.5e-8 3.4e-8         2d-wide 2.6e-7 1.0e-7 2.1e-7 4.4e-7
#   2d-deep 2.0e-7 1.3e-7 4.4e-7 6.1e-7          2d-big_grid 2.0e-7 9.0e-8 2.5e-7 1.9e-7     2d-sliced 1.5e-7 9.8e-8 1.2e-7 1.8e-7
#   3d-tiny 8.2e-8 8.0e-8 1.2e-7 4.9e-8          3d-small 1.4e-7 1.2e-7 1.9e-7 2.6e-7
# (with a 64-bit index sum for two inputs instead, the forward pass of six of the nine 2-D shapes is off by 0.1 to 0.6 of that magnitude)
# The tolerance is the project's fp32-chain tolerance (test_forward_is_bilinear_in_grid_and_relu_mlp): rtol 2e-4, and its absolute term
# 2e-5 times the largest reference magnitude of the compared array, since the widths (and with them the magnitudes) differ.
RTOL, ATOL = 2e-4, 2e-5


def _assert_close(got, want, what):
    top = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print("%s: worst deviation %.2g of the largest reference magnitude %.3g" % (what, err / max(top, 1e-300), top))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL * top, err_msg=what)


@pytest.mark.parametrize("dims,key", CASES, ids=CASE_IDS)
def test_oracle_matches_float64_restatement(orc, dims, key):
    """70 points -- the corners (0, 1) and (1, 1), points a little outside the unit square / cube and far outside it included: forward
    pass, encoding and the gradient of every parameter.  Makes the oracle a checked reference at the shapes the kernels are compared at."""
    cfg = _case(dims, key)
    levels = _levels64(orc, cfg, dims)
    p = _params(orc, cfg, seed=51, dims=dims)
    assert len(p) == _n_mlp(cfg) + sum(levels[2]) * cfg.n_features
    rng = np.random.default_rng(52)
    x = _points(rng, 70, dims, -0.05, 1.05, far=True)
    x[10:60] = rng.uniform(0, 1, (50, dims)).astype(np.float32)
    dl = rng.normal(size=(70, cfg.n_output)).astype(np.float32)
    out64, enc64, g64, w_sizes, g_sizes = _net64(cfg, dims, levels, p, x, dl)
    if dims == 3:
        out, acts = orc.net3_forward(cfg, p, x, want_acts=True)
    else:
        out, acts = orc.net_forward(cfg, p, x, want_acts=True)
    _assert_close(out, out64, "forward")
    _assert_close(acts[:, :enc64.shape[1]], enc64, "encoding")
    g = _backward(orc, cfg, dims, p, x, dl)
    off = 0
    for i, sz in enumerate(w_sizes + g_sizes):
        what = "matrix %d" % i if i < len(w_sizes) else "grid level %d" % (i - len(w_sizes))
        # an all-zero pass (a dead network, a level nothing reaches) must not count
        assert np.any(g[off:off + sz] != 0) and np.any(g64[off:off + sz] != 0), what
        _assert_close(g[off:off + sz], g64[off:off + sz], "gradient of " + what)
        off += sz
    assert off == len(g)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSED = {
    "17_levels": dict(n_levels=17, n_features_per_level=1),
    "24_levels": dict(n_levels=24, n_features_per_level=1),      # (an encoded width that passes: the level bound alone)
    "9_features": dict(n_levels=8, n_features_per_level=9),
    "enc_12": dict(n_levels=3, n_features_per_level=4),
    "enc_72": dict(n_levels=9, n_features_per_level=8),
    "4_neurons": dict(n_neurons=4),
    "12_neurons": dict(n_neurons=12),
    "72_neurons": dict(n_neurons=72),
    "0_hidden": dict(n_hidden_layers=0),
    "16_hidden": dict(n_hidden_layers=16),
    "0_outputs": dict(n_output=0),
    "65_outputs": dict(n_output=65),
    "base_0": dict(base_resolution=0),
    "scale_0.99": dict(per_level_scale=0.99),
    "scale_nan": dict(per_level_scale=float("nan")),
    "scale_inf": dict(per_level_scale=float("inf")),          # (0 * log2(inf): no grid size at all)
    "grid_past_1e9": dict(base_resolution=8192, per_level_scale=2.0),
}


@pytest.mark.parametrize("dims", [2, 3])
@pytest.mark.parametrize("key", list(REFUSED))
def test_net_create_refuses_shapes_outside_the_family(dims, key):
    """every bound of net_create_dims from just outside: WOST_ERR_UNSUPPORTED, a null handle and a message.  The shape checks -- the grid
    size among them -- come before the library looks for a device, so this runs without one."""
    from elaina_amd import capi
    from elaina_amd.guided import default_net_config as hip_default
    lib = capi.load()
    cfg = hip_default()
    for k, v in REFUSED[key].items():
        assert hasattr(cfg, k)
        setattr(cfg, k, v)
    handle = C.c_void_p(0xdead)
    create = lib.wost3_net_create if dims == 3 else lib.wost_net_create
    assert create(0, C.byref(cfg), 1, C.byref(handle)) == WOST_ERR_UNSUPPORTED
    assert not handle.value
    assert len(lib.wost_last_error()) > 0


# ---- GPU: the kernels of other shapes against the oracle ---------------------------------------------------------------------------
def _network(cfg, dims, seed=3):
    from elaina_amd.guided import GuidingNetwork
    return GuidingNetwork(_hip_cfg(cfg), seed=seed, dims=dims)


@pytest.mark.gpu
@pytest.mark.parametrize("dims,key", CASES, ids=CASE_IDS)
def test_gpu_network_shapes_match_oracle(orc, dims, key):
    """One handle per shape: inference (1, 65 and 1000 points), gradients (5 points: below one 64-point span; 4096 + 3: past the
    1024-point weight-gradient chunk and the 2048 / 4096-point grid chunks, ragged end) and two Adam steps of different batch sizes --
    outputs, gradients, weights and EMA weights equal to the oracle's bit for bit."""
    cfg = _case(dims, key)
    n_mlp = _n_mlp(cfg)
    p = _params(orc, cfg, seed=61, dims=dims, gscale=0.1)
    net = _network(cfg, dims)
    try:
        assert (net.n_params, net.n_mlp_params) == (len(p), n_mlp)
        net.set_params(p)
        rng = np.random.default_rng(62)
        for n in (1, 65, 1000):
            x = _points(rng, n, dims)
            got = net.inference(x)
            assert got.shape == (n, cfg.n_output)
            assert np.array_equal(got, _forward(orc, cfg, dims, p, x)[:, :cfg.n_output]), n
        for n in (5, 4096 + 3):
            x = _points(rng, n, dims)
            dl = rng.normal(size=(n, cfg.n_output)).astype(np.float32)
            net.train_step(x, dl, apply_update=False)
            got, want = net.gradients(), _backward(orc, cfg, dims, p, x, dl)
            assert np.any(want[:n_mlp] != 0) and np.any(want[n_mlp:] != 0)
            assert np.array_equal(got, want), (n, float(np.abs(got - want).max()))
            assert np.array_equal(net.params(), p)
        st = _opt_state(len(p))
        po = p.copy()
        for step, n in enumerate((3037, 64), 1):
            x = _points(rng, n, dims)
            dl = (rng.normal(size=(n, cfg.n_output)) * 128 / n).astype(np.float32)
            before = po.copy()
            net.train_step(x, dl, loss_scale=128.0)
            g = _backward(orc, cfg, dims, po, x, dl)
            assert np.array_equal(net.gradients(), g), step
            inf = _opt_step(orc, cfg, dims, po, st, g, step)
            got_p, got_inf = net.params(), net.inference_params()
            assert np.array_equal(got_p, po) and np.array_equal(got_inf, inf), step
            if step == 1 and dims == 2 and key in ("big_grid", "wide"):
                # 3037 points on a grid of 1.4 M / 0.7 M floats: most entries see no gradient, and optimizer_kernel leaves them alone
                idle = np.flatnonzero(g[n_mlp:] == 0) + n_mlp
                assert len(idle) > 0.5 * (len(p) - n_mlp)
                assert np.array_equal(got_p[idle], before[idle]) and not np.array_equal(got_p[:n_mlp], before[:n_mlp])
        # training and inference (EMA) weights differ now: both through the forward kernels
        assert not np.array_equal(po, inf)
        for n in (1, 65, 1000):
            x = _points(rng, n, dims)
            assert np.array_equal(net.inference(x), _forward(orc, cfg, dims, inf, x)[:, :cfg.n_output]), n
            assert np.array_equal(net.inference(x, use_inference_params=False), _forward(orc, cfg, dims, po, x)[:, :cfg.n_output]), n
    finally:
        net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["mfma_16x2", "sliced"])
def test_gpu_half_precision_is_refused_on_other_shapes(orc, key):
    """the half-precision kernels are built for 8 levels x 4 features, 3 x 64 only: both options answer WOST_ERR_UNSUPPORTED on any other
    shape -- one that runs on the matrix cores in fp32 (16 x 2) included -- and the handle goes on giving the oracle's fp32 outputs"""
    from elaina_amd.capi import WostError
    cfg = _cfg(SHAPES2[key])
    p = _params(orc, cfg, seed=71)
    net = _network(cfg, 2)
    try:
        net.set_params(p)
        x = _points(np.random.default_rng(72), 300, 2)
        want = _forward(orc, cfg, 2, p, x)[:, :cfg.n_output]
        for option in ("precision", "train_precision"):
            with pytest.raises(WostError, match=r"\(%d\)" % WOST_ERR_UNSUPPORTED):
                net.set_option(option, 16)
            assert np.array_equal(net.inference(x), want), option
            assert np.array_equal(net.inference(x, use_inference_params=False), want), option
    finally:
        net.close()


# ---- GPU: inputs outside the unit square ---------------------------------------------------------------------------------------------
OUTSIDE = [("reference", None), ("reference", "1"), ("mfma_16x2", None), ("deep", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("key,scalar", OUTSIDE, ids=["reference", "reference-scalar", "mfma_16x2", "deep"])
def test_gpu_outside_the_unit_square_matches_oracle(orc, monkeypatch, key, scalar):
    """The two-input mirror of test_gpu_net3_inference_and_training_match_oracle: points from [-0.05, 1.05]^2 and a few far outside.  There
    floor(scale * x + 0.5) is negative and the dense index wraps -- in 32 bits on both sides; on the levels whose entry
    count does not divide 2^32 a 64-bit sum reads another entry.  Inference and gradients bit for bit: MFMA kernels, the one-thread-per-
    point kernels at the same shape (WOST_NET_SCALAR=1), and two other shapes."""
    if scalar:
        monkeypatch.setenv("WOST_NET_SCALAR", scalar)
    cfg = default_net_config() if key == "reference" else _cfg(SHAPES2[key])
    n_mlp = _n_mlp(cfg)
    p = _params(orc, cfg, seed=81)
    net = _network(cfg, 2)
    try:
        net.set_params(p)
        rng = np.random.default_rng(82)
        x = _points(rng, 3000, 2, -0.05, 1.05, far=True)
        assert np.mean((x < 0).any(axis=1) | (x > 1).any(axis=1)) > 0.1
        want = _forward(orc, cfg, 2, p, x)[:, :cfg.n_output]
        got = net.inference(x)
        assert np.array_equal(got, want), float(np.mean((got != want).any(axis=1)))
        dl = rng.normal(size=(len(x), cfg.n_output)).astype(np.float32)
        net.train_step(x, dl, apply_update=False)
        got, want = net.gradients(), _backward(orc, cfg, 2, p, x, dl)
        assert np.array_equal(got[:n_mlp], want[:n_mlp]) and np.array_equal(got[n_mlp:], want[n_mlp:]), float(np.abs(got - want).max())
    finally:
        net.close()


@pytest.mark.gpu
def test_gpu_half_precision_inference_outside_the_unit_square(orc):
    """the comparison and the tolerances of test_gpu_half_precision_inference at points outside the unit square: the f16 image is indexed by
    the same rule (half_encode_level)"""
    cfg = default_net_config()
    net = _network(cfg, 2, seed=7)
    try:
        p = _rand_params(orc, cfg, seed=31, wscale=0.2, gscale=0.4)
        net.set_params(p)
        xy = _points(np.random.default_rng(83), 3000, 2, -0.05, 1.05, far=True)
        fp32 = net.inference(xy)
        assert np.array_equal(fp32, orc.net_forward(cfg, p, xy)[0][:, :33])
        net.set_option("precision", 16)
        half = net.inference(xy)
        emu = _half_network_numpy(orc, cfg, p, xy)
        scale = float(np.sqrt(np.mean(fp32 ** 2)))
        assert np.abs(half - emu).max() <= 4e-3 * scale, (float(np.abs(half - emu).max()), scale)
        assert np.mean(half == emu) > 0.9                                  # most outputs agree to the last f16 bit
        rel = float(np.sqrt(np.mean((half - fp32) ** 2))) / scale
        assert rel < 5e-3, rel
        assert np.array_equal(half, half.astype(np.float16).astype(np.float32))     # outputs are half-precision numbers
    finally:
        net.close()


# ---- GPU: guided solves with the guiding box inside the domain ----------------------------------------------------------------------
INNER_BOX = ((0.25, 0.2), (0.8, 0.7))
COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps")


def _lobed_params(orc, cfg):
    """the random network with pronounced lobes of test_gpu_frozen_network_matches_oracle"""
    rng = np.random.default_rng(3)
    n = orc.net_n_params(cfg)
    p = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    p[_n_mlp(cfg):] = rng.uniform(-1, 1, n - _n_mlp(cfg)).astype(np.float32)
    return p


def _starts_outside(prob, w, h, aabb):
    """evaluation points of the frame (core/evaluation_grid.h:27-33) that lie outside `aabb`: how many, and the largest distance of
    their network input normalize_coord(aabb, .) from the unit square"""
    s, cx, cy, ux, uy = [float(v) for v in prob.probe]
    px = (np.arange(w) * 2.0 / w - 1.0)[None, :] * np.ones((h, 1))
    py = (np.arange(h) * 2.0 / h - 1.0)[:, None] * np.ones((1, w))
    x, y = s * (px * uy + py * ux) + cx, s * (px * (-ux) + py * uy) + cy
    (x0, y0), (x1, y1) = aabb
    out = (x < x0) | (x > x1) | (y < y0) | (y > y1)
    infl = np.hypot(x1 - x0, y1 - y0) * 0.005
    nx, ny = (x - (x0 - infl)) / (x1 - x0 + 2 * infl), (y - (y0 - infl)) / (y1 - y0 + 2 * infl)
    past = np.maximum(np.maximum(-nx, nx - 1), np.maximum(-ny, ny - 1))
    return int(out.sum()), float(past[out].max())


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["1", "0"])
def test_gpu_frozen_network_with_an_inner_guiding_box_matches_oracle(oracle, monkeypatch, fused):
    """Walkers outside the guiding box are evaluated by the network like the others, at normalize_coord(box, .) outside [0, 1]^2, and
    never guided (handleOutShellPoint: routed to the mixture only inside the box, the pdf mixed only inside the box).  Field and counters
    bit for bit through the one-launch sample kernel and through the launches per depth (WOST_GUIDED_FUSED=0).
    What the network returns outside the box decides nothing but a comparison whose outcome is dropped there, so the field does not
    depend on the index rule; the assertions at the end establish that such positions ARE evaluated (guided depth 1: the network sees
    start positions only, and more of them than lie inside the box)."""
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    monkeypatch.setenv("WOST_GUIDED_FUSED", fused)
    prob = laplace_box()
    cfg = default_net_config()
    p = _lobed_params(oracle, cfg)
    w, h, spp = 48, 40, 3
    gi, ref = _gpu_and_oracle(oracle, prob, w, h, spp, 32, 0, params=p, aabb=INNER_BOX)
    try:
        assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
        for k in COUNTERS:
            assert gi.last_stats[k] == ref[k], k
        assert ref["guided_steps"] > 0
        assert np.array_equal(gi.network.params(), p)
    finally:
        gi.close()
    n_outside, past = _starts_outside(prob, w, h, INNER_BOX)
    assert n_outside > w * h // 2 and past > 0.3          # most of the frame, up to a third of the box's width outside it
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=1, trainSppCount=0, maxWalkingDepth=32, epsilonShell=1e-3,
                                  maxGuidedDepthInTrainingPhase=1, maxGuidedDepthInGuidingPhase=1)
    gi = GuidedIntegrator(prob, st, INNER_BOX, seed=7)
    try:
        gi.network.set_params(p)
        gi.solve()
        assert w * h - n_outside < gi.last_stats["net_points"] <= w * h, (gi.last_stats["net_points"], n_outside)
    finally:
        gi.close()


@pytest.mark.gpu
def test_gpu_training_with_an_inner_guiding_box_matches_oracle(oracle):
    """test_gpu_training_end_to_end_matches_oracle with the guiding box inside the domain: records outside the box stay out of the training
    set, walkers outside it are evaluated and walk on uniformly -- field, counters and the trained weights against the oracle"""
    prob = laplace_box()
    w = h = 48
    gi, ref = _gpu_and_oracle(oracle, prob, w, h, 32, 32, 16, dump=False, aabb=INNER_BOX)
    try:
        st = gi.last_stats
        assert st["optimizer_steps"] == ref["optimizer_steps"] > 0
        for k in COUNTERS + ("train_samples",):
            assert st[k] == ref[k], k
        assert ref["guided_steps"] > 0
        assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
        assert st["walks_absorbed"] + st["walks_truncated"] == st["walks_started"] == w * h * 32
        assert np.array_equal(gi.network.params(), ref["params"])
        assert np.abs(gi.network.params() - gi.network.inference_params()).max() > 0
    finally:
        gi.close()
    assert _starts_outside(prob, w, h, INNER_BOX)[0] > w * h // 2


@pytest.mark.gpu
def test_gpu_guided_solve_on_another_network_shape_matches_oracle(oracle):
    """4 levels x 4 features, 2 x 32 neurons: net_f32_view declines, so every depth is a launch of its own with the one-thread-per-point
    forward kernel in between, and the training sample runs the scalar backward pass with a gradient plan of another shape.  Field,
    counters and weights against the oracle bit for bit."""
    cfg = _cfg((4, 4, 8, 1.405, 32, 2, 33))
    prob = laplace_box()
    gi, ref = _gpu_and_oracle(oracle, prob, 48, 40, 3, 32, 1, dump=False, cfg=cfg)
    try:
        st = gi.last_stats
        assert gi.network.n_params == oracle.net_n_params(cfg)
        assert st["optimizer_steps"] == ref["optimizer_steps"] > 0
        for k in COUNTERS + ("train_samples",):
            assert st[k] == ref[k], k
        assert ref["guided_steps"] > 0
        assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
        assert np.array_equal(gi.network.params(), ref["params"])
    finally:
        gi.close()
