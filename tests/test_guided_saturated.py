"""The directional mixtures at the inputs their code is written to survive (wost_vmm_device.h, wost_vmm3_device.h and the copies in
guided_sample_kernel, the per-depth guided kernels, g3_fused_kernel and the two loss-gradient kernels): lambda and kappa are
exp(clamp(x, -10, 15)), log_bessel changes branch at kappa 3.75, vm_dlog_dkappa has a double-precision branch, the 3-D kappa
derivative is a fitted parabola below 1, and the lobe pick falls back to lobe 0 when no weight catches the draw.

The networks of the other guided tests stay far from all of that: at 4 096 uniform points MLP weights in +-0.3 give raw outputs
in [-2.70, 2.20] in 2-D (log kappa <= 1.82: kappa <= 6.2, 0.03 % of the lobes past 3.75) and within +-0.83 in 3-D (log kappa <=
0.65: kappa <= 1.9), which test_the_mild_networks_of_the_other_tests_touch_no_edge asserts.  With weights in +-0.6 the reference-shaped network gives raw outputs in
[-43, 35], with +-1.0 in [-333, 271]: every clamp edge is crossed by a good share of the lobes (checked below on the CPU, so that
a pass on the GPU means something), and half precision -- the reference's own precision -- gets there sooner.

  1. frozen saturated networks through every form of the guided kernels, bit for bit against the oracle (field and counters);
     half precision: fused = per depth = a second solve of the handle;
  2. training that starts from a saturated network: field, training set, counters, optimizer steps and weights, bit for bit;
  3. the batch entry points over their whole input domain: saturated raw outputs, the kappa values at which the code changes
     path with their float neighbours, cosines at and beyond +-1, sampling at kappa = e^15, sizes at the block edges, non-finite
     raw outputs (density only: a wrong clamp would turn the rejection sampler into an endless loop), and the pick that no
     weight catches.  Equality of bits in 2-D as in 3-D: both sides share the deterministic exp / log / sin / cos / acos.

Every oracle solve is computed once per process (_once) and shared by the forms of the kernels and by the CPU conditions."""
import math

import numpy as np
import pytest

from oracle.oracle import default_net_config, default_net_config3, guided_settings3
from test_guided_3d import AABB3, COUNTERS, _cfg, _gpu_and_oracle3, _rand_params3, _with_env, mixed_cube
from test_guided_integrator import AABB, EPS, _gpu_and_oracle, laplace_box
from test_guided_refill import ORACLE_KEYS, _gpu, _matches_oracle, _oracle, _same

_ONCE = {}


def _once(key, make):
    if key not in _ONCE:
        _ONCE[key] = make()
    return _ONCE[key]


# ---- the saturated networks ---------------------------------------------------------------------------------------------------
WSCALES2 = [0.6, 1.0]
FRACTIONS = [(0.0, 0.0), (0.5, 0.5)]
LEVELS3 = [4, 8]          # four levels: the scalar network kernels and the launches per depth; eight: the matrix kernels and g3_fused_kernel


def _params2(oracle, wscale):
    # test_gpu_frozen_network_matches_oracle's network with larger MLP weights
    rng = np.random.default_rng(3)
    n = oracle.net_n_params(default_net_config())
    p = rng.uniform(-wscale, wscale, n).astype(np.float32)
    p[13312:] = rng.uniform(-1, 1, n - 13312).astype(np.float32)
    return p


def _cfg3(levels):
    return _cfg() if levels == 4 else default_net_config3()


def _params3(oracle, levels):
    return _rand_params3(oracle, _cfg3(levels), seed=3, wscale=1.0, gscale=1.0)


def _frozen_scene2(uf):
    return dict(prob=laplace_box(), w=48, h=40, spp=3, train=0, depth=32, eps=EPS, aabb=AABB, batch=2048, min_batch=512, uf=uf)


def _frozen_ref2(oracle, wscale, uf):
    return _once(("frozen2", wscale, uf), lambda: _oracle(oracle, _frozen_scene2(uf), _params2(oracle, wscale)))


TRAIN2 = dict(w=48, h=48, spp=4, train_spp=2, depth=32, batch=2048, min_batch=512)
FROZEN3 = dict(w=40, h=32, spp=2, depth=48, train_spp=0)
TRAIN3 = dict(w=40, h=40, spp=4, depth=48, train_spp=2, batch=1024, min_batch=256)


def _oracle_solve2(oracle, params, w, h, spp, depth, train_spp, batch, min_batch):
    from oracle.oracle import guided_settings
    gs = guided_settings(w, h, spp, depth, EPS, AABB[0], AABB[1], train_spp_count=train_spp, batch_size=batch, min_batch_size=min_batch)
    trained = params.copy()
    ref = oracle.solve_guided(laplace_box().as_dict(), gs, default_net_config(), trained, threads=16, dump_spp=train_spp - 1)
    ref["params"] = trained
    return ref


def _oracle_solve3(oracle, levels, w, h, spp, depth, train_spp, batch=1024, min_batch=256):
    gs = guided_settings3(w, h, spp, depth, EPS, AABB3[0], AABB3[1], train_spp_count=train_spp, batch_size=batch, min_batch_size=min_batch)
    trained = _params3(oracle, levels)
    ref = oracle.solve_guided3(mixed_cube(), gs, _cfg3(levels), trained, threads=16, dump_spp=train_spp - 1)
    ref["params"] = trained
    return ref


def _train_ref2(oracle):
    return _once("train2", lambda: _oracle_solve2(oracle, _params2(oracle, 0.6), **TRAIN2))


def _frozen_ref3(oracle, levels):
    return _once(("frozen3", levels), lambda: _oracle_solve3(oracle, levels, **FROZEN3))


def _train_ref3(oracle):
    return _once("train3", lambda: _oracle_solve3(oracle, 4, **TRAIN3))


# ---- conditions, on the CPU: the networks do saturate, and the oracle walks through it ---------------------------------------------
def _edge_shares(raw, stride):
    """the share of points x lobes whose lambda slot / log kappa slot lies beyond each of the four clamp edges"""
    lam, kap = raw[:, 0:8 * stride:stride], raw[:, 1:8 * stride:stride]
    return {"lambda > 15": float((lam > 15).mean()), "lambda < -10": float((lam < -10).mean()),
            "log kappa > 15": float((kap > 15).mean()), "log kappa < -10": float((kap < -10).mean())}


@pytest.mark.parametrize("wscale", WSCALES2)
def test_the_2d_networks_cross_every_clamp_edge(oracle, wscale):
    """measured: 1.8 %, 2.0 %, 0.53 %, 11 % with weights in +-0.6; 40 %, 35 %, 29 %, 50 % with +-1.0"""
    xy = np.random.default_rng(0).uniform(0.0, 1.0, (4096, 2)).astype(np.float32)
    raw, _ = oracle.net_forward(default_net_config(), _params2(oracle, wscale), xy)
    shares = _edge_shares(raw, 4)
    print(wscale, float(raw[:, :33].min()), float(raw[:, :33].max()), shares)
    assert np.isfinite(raw).all() and np.abs(raw).max() < 6e4             # no overflow in half precision either
    assert all(s >= 1e-3 for s in shares.values()), shares


@pytest.mark.parametrize("levels", LEVELS3)
def test_the_3d_networks_cross_every_clamp_edge(oracle, levels):
    """measured with four levels: 29 %, 25 %, 15 %, 31 %, and 26 % of the lobes with log kappa in (-10, 0): the fitted parabola"""
    x = np.random.default_rng(0).uniform(0.0, 1.0, (4096, 3)).astype(np.float32)
    raw = oracle.net3_forward(_cfg3(levels), _params3(oracle, levels), x)
    shares = _edge_shares(raw, 5)
    below_one = float(((raw[:, 1:40:5] > -10) & (raw[:, 1:40:5] < 0)).mean())
    print(levels, float(raw[:, :41].min()), float(raw[:, :41].max()), shares, below_one)
    assert np.isfinite(raw).all()
    assert all(s >= 1e-3 for s in shares.values()) and below_one >= 1e-3, (shares, below_one)


def test_the_mild_networks_of_the_other_tests_touch_no_edge(oracle):
    """the frozen networks of test_guided_integrator.py, test_guided_refill.py (MLP weights in +-0.3, grid part +-1) and
    test_guided_3d.py (wscale 0.3, gscale 1.0) at the same 4 096 points: the ranges their docstrings state"""
    xy = np.random.default_rng(0).uniform(0.0, 1.0, (4096, 2)).astype(np.float32)
    raw = oracle.net_forward(default_net_config(), _params2(oracle, 0.3), xy)[0][:, :33]
    log_kappa = raw[:, 1:32:4]
    print("2-D", float(raw.min()), float(raw.max()), float(log_kappa.max()), float((log_kappa > math.log(3.75)).mean()))
    assert -2.70 <= raw.min() and raw.max() <= 2.20 and 1.81 < log_kappa.max() <= 1.82
    assert 0 < (log_kappa > math.log(3.75)).mean() < 1e-3
    x = np.random.default_rng(0).uniform(0.0, 1.0, (4096, 3)).astype(np.float32)
    raw = oracle.net3_forward(_cfg(), _rand_params3(oracle, _cfg(), seed=3, wscale=0.3, gscale=1.0), x)[:, :41]
    print("3-D", float(raw.min()), float(raw.max()), float(raw[:, 1:40:5].max()))
    assert np.abs(raw).max() <= 0.83 and 0.64 < raw[:, 1:40:5].max() <= 0.65


def test_the_oracle_walks_through_the_saturated_networks(oracle):
    """every oracle solve the GPU tests below compare with: a finite field and at least 1 000 guided steps in it -- the floor
    test_gpu_guided3_reference_network_fused_and_per_depth asks of the same 3-D frame (the eight-level network, the only
    saturated one g3_fused_kernel sees, has the fewest: 5 514 of 55 049 walk steps)"""
    refs = {("frozen2", ws, uf): _frozen_ref2(oracle, ws, uf)[0] for ws in WSCALES2 for uf in FRACTIONS}
    refs.update({("frozen3", lv): _frozen_ref3(oracle, lv) for lv in LEVELS3})
    refs["train2"], refs["train3"] = _train_ref2(oracle), _train_ref3(oracle)
    for key, ref in refs.items():
        print(key, {k: ref[k] for k in ORACLE_KEYS})
        assert np.isfinite(ref["field"]).all(), key
        assert ref["guided_steps"] >= 1000 and ref["walks_started"] > 0, key
    for key in ("train2", "train3"):
        assert refs[key]["optimizer_steps"] > 0 and refs[key]["train_samples"] > 0 and np.isfinite(refs[key]["params"]).all(), key
        assert all(np.isfinite(v).all() for v in refs[key]["train_set"].values()), key


# ---- 1. frozen saturated networks through every form of the guided kernels ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("uf", FRACTIONS, ids=lambda u: "uf%g" % u[0])
@pytest.mark.parametrize("wscale", WSCALES2)
def test_gpu_frozen_saturated_network_2d(oracle, monkeypatch, capfd, wscale, uf):
    """the fused kernel, the launches per depth and the fused kernel on one block (each lane walks three pixels, lobes prepared
    for other lanes' walkers): field, counters and the untouched weights against the oracle, bit for bit"""
    sc, p = _frozen_scene2(uf), _params2(oracle, wscale)
    ref, p_ref = _frozen_ref2(oracle, wscale, uf)
    assert ref["guided_steps"] > 0 and ref["optimizer_steps"] == 0 and np.isfinite(ref["field"]).all()
    fused = _gpu(monkeypatch, sc, params=p)[0][0]
    _matches_oracle(fused, ref, p_ref, "fused")
    assert np.array_equal(fused[2], p)
    _matches_oracle(_gpu(monkeypatch, sc, {"WOST_GUIDED_FUSED": 0}, params=p)[0][0], ref, p_ref, "per depth")
    assert sc["w"] * sc["h"] >= 2 * 640
    _matches_oracle(_gpu(monkeypatch, sc, {"WOST_GUIDED_MAX_BLOCKS": 1}, params=p, capfd=capfd, blocks=1)[0][0], ref, p_ref, "one block")


@pytest.mark.gpu
@pytest.mark.parametrize("levels", LEVELS3)
def test_gpu_frozen_saturated_network_3d(oracle, levels):
    """WOST3_G_FUSED 0 / 1 and WOST3_WAVE 0 / 1 (the reference's eight levels: g3_fused_kernel against the launches per depth;
    four levels: the launches per depth with the scalar network kernels, whatever is asked for)"""
    ref = _frozen_ref3(oracle, levels)
    p = _params3(oracle, levels)
    for fused in ("0", "1"):
        for wave in ("0", "1"):
            what = "fused %s wave %s" % (fused, wave)
            gi, _ = _with_env({"WOST3_G_FUSED": fused, "WOST3_WAVE": wave},
                              lambda: _gpu_and_oracle3(oracle, mixed_cube(), params=p, cfg=_cfg3(levels), ref=ref, **FROZEN3))
            assert np.array_equal(gi.solution, ref["field"]), (what, float(np.abs(gi.solution - ref["field"]).max()))
            for k in COUNTERS:
                assert gi.last_stats[k] == ref[k], (what, k, gi.last_stats[k], ref[k])
            assert np.array_equal(gi.network.params(), p), what
            if levels == 8 and fused == "1":
                assert gi.last_stats["kernel_launches"] <= FROZEN3["spp"] * 2 + 2, gi.last_stats["kernel_launches"]
            gi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("uf", FRACTIONS, ids=lambda u: "uf%g" % u[0])
def test_gpu_frozen_saturated_network_half_precision_2d(oracle, monkeypatch, uf):
    """weights in +-1.0 (raw outputs within +-340: no f16 overflow) with the half-precision network: a finite field, the fused
    kernel equal to the launches per depth, and a second solve of the same handle equal to the first.  No oracle in this mode."""
    sc, p = _frozen_scene2(uf), _params2(oracle, 1.0)
    fused = _gpu(monkeypatch, sc, precision=16, params=p, solves=2)[0]
    per_depth = _gpu(monkeypatch, sc, {"WOST_GUIDED_FUSED": 0}, precision=16, params=p, solves=2)[0]
    assert np.isfinite(fused[0][0]).all() and fused[0][1]["guided_steps"] > 0 and fused[0][1]["optimizer_steps"] == 0
    _same(fused[0], per_depth[0], "fused = per depth")
    _same(fused[0], fused[1], "second solve, fused")
    _same(per_depth[0], per_depth[1], "second solve, per depth")


# ---- 2. training that starts from a saturated network ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_training_from_a_saturated_network_2d(oracle):
    """two trained and two guided samples from weights in +-0.6: walks, records, batches, gradients and Adam steps, bit for bit"""
    ref = _train_ref2(oracle)
    gi, _ = _gpu_and_oracle(oracle, laplace_box(), TRAIN2["w"], TRAIN2["h"], TRAIN2["spp"], TRAIN2["depth"], TRAIN2["train_spp"],
                            batch=TRAIN2["batch"], min_batch=TRAIN2["min_batch"], params=_params2(oracle, 0.6), ref=ref)
    st = gi.last_stats
    for k in ORACLE_KEYS:
        assert st[k] == ref[k], (k, st[k], ref[k])
    assert ref["optimizer_steps"] > 0 and ref["guided_steps"] > 0
    assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
    ts, to = gi.train_set(), ref["train_set"]
    assert len(ts["xy"]) == len(to["xy"]) > 0
    for k in ("xy", "dir", "solution", "dir_pdf", "normal", "on_neumann"):
        assert np.array_equal(ts[k], to[k]), k
    assert np.isfinite(ref["params"]).all() and np.array_equal(gi.network.params(), ref["params"])
    gi.close()


@pytest.mark.gpu
def test_gpu_training_from_a_saturated_network_3d(oracle):
    ref = _train_ref3(oracle)
    gi, _ = _gpu_and_oracle3(oracle, mixed_cube(), params=_params3(oracle, 4), ref=ref, **TRAIN3)
    for k in COUNTERS + ("train_samples", "optimizer_steps"):
        assert gi.last_stats[k] == ref[k], (k, gi.last_stats[k], ref[k])
    assert ref["optimizer_steps"] > 0 and ref["guided_steps"] > 0
    assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
    ts, to = gi.train_set(), ref["train_set"]
    assert len(ts["xyz"]) == len(to["xyz"]) > 0
    for k in ("xyz", "dir", "solution", "dir_pdf", "normal", "on_neumann"):
        assert np.array_equal(ts[k], to[k]), k
    assert np.isfinite(ref["params"]).all() and np.array_equal(gi.network.params(), ref["params"])
    gi.close()


# ---- 3. the batch entry points over their whole input domain ----------------------------------------------------------------------------
F32 = np.float32
E15, EM10 = F32(math.exp(15.0)), F32(math.exp(-10.0))
U_MAX = F32(1.0) - F32(2.0 ** -23)            # the largest float a draw can be (core/sampler.h:87-98)


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _neighbours(values):
    """every value with the floats next to it on both sides"""
    v = np.asarray(values, np.float32)
    return np.concatenate([v, np.nextafter(v, F32(np.inf)), np.nextafter(v, F32(-np.inf))])


# the kappa values at which the code changes path: the clamp's ends, the 2-D uniform switch, the Bessel branch (and the branch of
# vm_dlog_dkappa), the 3-D parabola and the 3-D M_EPSILON
KAPPAS = _neighbours([E15, EM10, 1e-3, 3.75, 1.0, 1e-5])
COSINES = _neighbours([1.0, -1.0]).tolist() + [0.0, 0.5, -0.25]


def _records(rng, n, dims):
    """direction, Li, dirPdf, Neumann flag and normal of n training records"""
    return (_unit(rng.normal(size=(n, dims))), rng.uniform(0.0, 1.0, n).astype(np.float32), rng.uniform(0.05, 0.6, n).astype(np.float32),
            (rng.uniform(size=n) < 0.3).astype(np.uint8), _unit(rng.normal(size=(n, dims))))


def _saturated_raw(rng, n, dims):
    """raw outputs of n points (8 lobes x (lambda, log kappa, mean vector) + the selection logit) with the lambda and log kappa
    slots uniform in [-14, 19]: 12 % of them beyond either end of the clamp"""
    stride = 2 + dims
    raw = rng.normal(0.0, 1.5, size=(n, 8 * stride + 1)).astype(np.float32)
    raw[:, 0:8 * stride:stride] = rng.uniform(-14.0, 19.0, size=(n, 8))
    raw[:, 1:8 * stride:stride] = rng.uniform(-14.0, 19.0, size=(n, 8))
    return raw


def _edge_raw(rng, n, dims):
    """the same with the lambda and log kappa slots drawn from the values at which exp(clamp(x)) changes path: the ends of the
    clamp and the logarithms of 3.75, 1 and 1e-3, each with a few floats on both sides, and values far outside"""
    stride = 2 + dims
    steps = np.arange(-6, 7)
    edges = [F32(15.0) + steps * np.spacing(F32(8.0)), F32(-10.0) + steps * np.spacing(F32(8.0)),
             F32(math.log(3.75)) + steps * np.spacing(F32(1.0)), steps * np.spacing(F32(0.5)),
             F32(math.log(1e-3)) + steps * np.spacing(F32(4.0)), [16.0, 40.0, -11.0, -40.0, 3e38, -3e38, 0.0]]
    edges = np.concatenate([np.asarray(e, np.float32) for e in edges])
    raw = rng.normal(0.0, 1.5, size=(n, 8 * stride + 1)).astype(np.float32)
    raw[:, 0:8 * stride:stride] = rng.choice(edges, size=(n, 8))
    raw[:, 1:8 * stride:stride] = rng.choice(edges, size=(n, 8))
    return raw


def _mixture_calls(dims):
    """(oracle's, device's) density + sample and loss gradients of the mixture in `dims` dimensions"""
    if dims == 2:
        from elaina_amd import guided
        return "vmm_pdf_sample", "vmm_loss_gradients", guided
    from elaina_amd import integrator3d
    return "vmm3_pdf_sample", "vmm3_loss_gradients", integrator3d


def _assert_mixture_equal(oracle, dims, raw, rng, sample=True, equal_nan=False):
    """density, sampled direction and loss gradients of the rows `raw` on the device against the oracle, bit for bit; returns the
    oracle's (pdf, dir, gradients, likelihood)"""
    pdf_sample, loss_gradients, dev = _mixture_calls(dims)
    n, m = len(raw), 8 * (2 + dims)
    wi, li, dir_pdf, on_n, normal = _records(rng, n, dims)
    seed = rng.integers(0, 2 ** 62, n).astype(np.uint64)
    rp, rd = getattr(oracle, pdf_sample)(raw[:, :m], wi, seed, sample=sample)
    gp, gd = getattr(dev, pdf_sample)(raw[:, :m], wi, seed, sample=sample)
    assert np.array_equal(gp, rp, equal_nan=equal_nan), (n, float(np.nanmax(np.abs(gp - rp))))
    if sample:
        assert np.array_equal(gd, rd, equal_nan=equal_nan), (n, float(np.nanmax(np.abs(gd - rd))))
    else:
        assert gd is None and rd is None
    rg, rl = getattr(oracle, loss_gradients)(raw, wi, li, dir_pdf, on_n, normal)
    gg, gl = getattr(dev, loss_gradients)(raw, wi, li, dir_pdf, on_n, normal)
    assert np.array_equal(gg, rg, equal_nan=equal_nan), (n, float(np.nanmax(np.abs(gg - rg))))
    assert np.array_equal(gl, rl, equal_nan=equal_nan), (n, float(np.nanmax(np.abs(gl - rl))))
    return rp, rd, rg, rl


@pytest.mark.parametrize("dims", [2, 3])
def test_the_oracle_stays_finite_on_saturated_mixtures(oracle, dims):
    """measured in 2-D at n = 20 000: every density finite, the largest 357, 0.08 % exact zeros, every direction a unit vector"""
    rng = np.random.default_rng(11)
    raw = _saturated_raw(rng, 20000, dims)
    slots = np.concatenate([raw[:, 0:8 * (2 + dims):2 + dims], raw[:, 1:8 * (2 + dims):2 + dims]])
    assert (slots > 15).mean() > 0.1 and (slots < -10).mean() > 0.1
    wi, li, dir_pdf, on_n, normal = _records(rng, len(raw), dims)
    pdf_sample, loss_gradients = ("vmm_pdf_sample", "vmm_loss_gradients") if dims == 2 else ("vmm3_pdf_sample", "vmm3_loss_gradients")
    pdf, d = getattr(oracle, pdf_sample)(raw[:, :8 * (2 + dims)], wi, rng.integers(0, 2 ** 62, len(raw)).astype(np.uint64))
    print(dims, float(pdf.max()), float((pdf == 0).mean()))
    assert np.isfinite(pdf).all() and (pdf >= 0).all() and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-5)
    g, lk = getattr(oracle, loss_gradients)(raw, wi, li, dir_pdf, on_n, normal)
    assert np.isfinite(g).all() and np.isfinite(lk).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [2, 3])
def test_hip_saturated_mixtures_match_oracle(oracle, dims):
    rng = np.random.default_rng(12)
    pdf, d, g, lk = _assert_mixture_equal(oracle, dims, _saturated_raw(rng, 20000, dims), rng)
    assert np.isfinite(pdf).all() and np.isfinite(d).all() and np.isfinite(g).all() and np.isfinite(lk).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [2, 3])
def test_hip_mixtures_at_the_edges_of_the_activations_match_oracle(oracle, dims):
    rng = np.random.default_rng(13)
    pdf, d, g, lk = _assert_mixture_equal(oracle, dims, _edge_raw(rng, 4099, dims), rng)
    assert np.isfinite(pdf).all() and np.isfinite(d).all() and np.isfinite(g).all() and np.isfinite(lk).all()


@pytest.mark.gpu
def test_hip_von_mises_at_the_branch_points_matches_oracle(oracle):
    """log I0, log I1, the log density and its kappa derivative at every pair of KAPPAS x COSINES (a cosine one ulp beyond +-1 is
    what a dot product of unit vectors gives), and the rejection sampler at the same kappas: e^15 is the most the clamp lets
    through"""
    from elaina_amd import guided
    kappa = np.repeat(KAPPAS, len(COSINES))
    cos = np.tile(np.asarray(COSINES, np.float32), len(KAPPAS))
    got, ref = guided.vonmises_eval(kappa, cos), oracle.vonmises_eval(kappa, cos)
    for k in ("log_i0", "log_i1", "log_pdf", "dlog_dkappa"):
        assert np.isfinite(ref[k]).all(), k
        assert np.array_equal(got[k], ref[k]), (k, float(np.abs(got[k] - ref[k]).max()))
    rng = np.random.default_rng(14)
    kappa = np.concatenate([np.tile(KAPPAS, 60), np.full(920, E15)]).astype(np.float32)
    assert len(kappa) == 2000
    seed = rng.integers(0, 2 ** 62, len(kappa)).astype(np.uint64)
    ref = oracle.vonmises_sample(kappa, seed, 8)
    assert np.isfinite(ref).all() and np.abs(ref[kappa >= 1e6]).max() < 0.01
    got = guided.vonmises_sample(kappa, seed, 8)
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())


@pytest.mark.gpu
def test_hip_vmf_at_the_branch_points_matches_oracle(oracle):
    """the lobe's density at every pair of KAPPAS x COSINES and its sampler at the same kappas.  Unit length is asserted for the
    kappas a mixture can have (>= e^-10) and for the uniform branch below 1e-5; between the two, which only a direct call reaches,
    1 + log(1 + ...) / kappa (util/vmf.h:49) cancels so far that the oracle's cosine leaves [-1, 1] by up to 0.3 % at kappa = 1e-5"""
    from elaina_amd import integrator3d
    kappa = np.repeat(KAPPAS, len(COSINES))
    cos = np.tile(np.asarray(COSINES, np.float32), len(KAPPAS))
    ref = oracle.vmf_eval(kappa, cos)
    assert np.isfinite(ref).all()
    assert np.array_equal(integrator3d.vmf_eval(kappa, cos), ref)
    rng = np.random.default_rng(15)
    kappa = np.concatenate([np.tile(KAPPAS, 60), np.full(920, E15)]).astype(np.float32)
    mu = _unit(rng.normal(size=(len(kappa), 3)))
    mu[:60] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 60)] * rng.choice([-1.0, 1.0], (60, 1)).astype(np.float32)
    seed = rng.integers(0, 2 ** 62, len(kappa)).astype(np.uint64)
    ref = oracle.vmf_sample(kappa, mu, seed, 8)
    direct_only = (kappa >= F32(1e-5)) & (kappa < F32(0.999) * EM10)
    assert np.isfinite(ref).all() and np.allclose(np.linalg.norm(ref, axis=2)[~direct_only], 1.0, atol=2e-6)
    assert ((ref * mu[:, None, :]).sum(2)[kappa >= 1e6] > 0.9999).all()
    assert np.array_equal(integrator3d.vmf_sample(kappa, mu, seed, 8), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_hip_batch_sizes_at_the_block_edges_match_oracle(oracle, n):
    """blocks of 128 (the 2-D loss gradients, staged through LDS with a partial last block), 256 (the other kernels) and 64 (the
    von Mises sampler): one row, a block less one row, a full block, a block and one row, two blocks and one row"""
    from elaina_amd import guided, integrator3d
    rng = np.random.default_rng(16)
    for dims in (2, 3):
        _assert_mixture_equal(oracle, dims, _saturated_raw(rng, n, dims), rng)
    kappa = np.exp(rng.uniform(-12.0, 15.0, n)).astype(np.float32)
    cos = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    seed = rng.integers(0, 2 ** 62, n).astype(np.uint64)
    mu = _unit(rng.normal(size=(n, 3)))
    # the oracle first: what the CPU cannot finish never reaches a rejection loop on the device
    ref, ref_theta = oracle.vonmises_eval(kappa, cos), oracle.vonmises_sample(kappa, seed, 3)
    ref_pdf3, ref_dir3 = oracle.vmf_eval(kappa, cos), oracle.vmf_sample(kappa, mu, seed, 3)
    assert np.isfinite(ref_theta).all() and np.isfinite(ref_pdf3).all() and np.isfinite(ref_dir3).all()
    got = guided.vonmises_eval(kappa, cos)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(guided.vonmises_sample(kappa, seed, 3), ref_theta)
    assert np.array_equal(integrator3d.vmf_eval(kappa, cos), ref_pdf3)
    assert np.array_equal(integrator3d.vmf_sample(kappa, mu, seed, 3), ref_dir3)


def _non_finite_raw(rng, n, dims, slots):
    """saturated rows with NaN, +inf and -inf in a quarter of the lambda and log kappa slots (`slots` = "activations") or of the
    mean vectors' components ("means")"""
    stride = 2 + dims
    raw = _saturated_raw(rng, n, dims)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    cols = [c for k in range(8) for c in ((stride * k, stride * k + 1) if slots == "activations" else range(stride * k + 2, stride * k + stride))]
    sub = raw[:, cols]
    hit = rng.uniform(size=sub.shape) < 0.25
    sub[hit] = rng.choice(bad, size=int(hit.sum()))
    raw[:, cols] = sub
    return raw


@pytest.mark.parametrize("dims", [2, 3])
def test_the_clamp_makes_non_finite_activations_finite(oracle, dims):
    """fmaxf(fminf(x, 15), -10) gives 15 for NaN and +inf, -10 for -inf: the oracle's density stays finite.  NaN or inf in a mean
    vector makes the 2-D density NaN (a lobe with kappa < 1e-3 aside); the 3-D lobe's min(0, cosTheta - 1) (util/vmf.h:30) is 0 for a
    NaN cosine, so that density stays finite, at the lobe's peak"""
    rng = np.random.default_rng(17)
    name = "vmm_pdf_sample" if dims == 2 else "vmm3_pdf_sample"
    raw = _non_finite_raw(rng, 2000, dims, "activations")
    assert not np.isfinite(raw).all()
    wi = _records(rng, len(raw), dims)[0]
    pdf, d = getattr(oracle, name)(raw[:, :8 * (2 + dims)], wi, None, sample=False)
    assert d is None and np.isfinite(pdf).all() and (pdf >= 0).all()
    raw = _non_finite_raw(rng, 2000, dims, "means")
    pdf, _ = getattr(oracle, name)(raw[:, :8 * (2 + dims)], wi, None, sample=False)
    assert np.isfinite(pdf).any() and (np.isnan(pdf).mean() > 0.5 if dims == 2 else np.isfinite(pdf).all())


@pytest.mark.gpu
@pytest.mark.parametrize("slots", ["activations", "means"])
@pytest.mark.parametrize("dims", [2, 3])
def test_hip_non_finite_raw_outputs_match_oracle(oracle, dims, slots):
    """the density alone (a null sample_dir through the C-ABI: nothing is sampled from such rows) and the loss gradients; where a
    mean vector is not finite there are NaN results, on both sides alike"""
    rng = np.random.default_rng(18)
    pdf, _, g, _ = _assert_mixture_equal(oracle, dims, _non_finite_raw(rng, 2000, dims, slots), rng, sample=False, equal_nan=slots == "means")
    if slots == "activations":
        assert np.isfinite(pdf).all() and np.isfinite(g).all()


# ---- the pick that no weight catches ------------------------------------------------------------------------------------------------
# seeds s < 2^26 whose stream setSeed(s, 1) gives U_MAX as its first draw -- found with _first_draw_bits below, confirmed with the
# oracle's generator: only with that draw can u outlast the running subtraction of eight float weights that sum to one
MAX_DRAW_SEEDS = (26240590, 36926204, 39798598, 42053371, 55848468, 56203965, 63840319)


def _first_draw_bits(seed):
    """the 23 mantissa bits of the first float of the stream setSeed(seed, 1) (core/sampler.h:20-27,65-72,87-98), for an array of
    uint64 seeds: inc = 3, state 0 -> 3 -> 3 + seed -> (3 + seed) M + 3, and the draw is made from that state"""
    M = np.uint64(0x5851f42d4c957f2d)
    with np.errstate(over="ignore"):
        s = (seed + np.uint64(3)) * M + np.uint64(3)
        xs = (((s >> np.uint64(18)) ^ s) >> np.uint64(27)).astype(np.uint32)
        rot = (s >> np.uint64(59)).astype(np.uint32)
        r = (xs >> rot) | (xs << ((np.uint32(0) - rot) & np.uint32(31)))
    return r >> np.uint32(9)


def _fall_through_batch(dims, per_seed=300):
    """rows with N(0, 1) lambda slots and narrow lobes (kappa = e^8: a sample lies within a degree or two of its lobe's mean),
    each paired with a seed whose first draw is U_MAX; and the rows for which a float32 restatement of the pick loop finds no lobe"""
    rng = np.random.default_rng(19)
    n, stride = per_seed * len(MAX_DRAW_SEEDS), 2 + dims
    raw = rng.normal(0.0, 1.0, size=(n, 8 * stride)).astype(np.float32)
    raw[:, 1::stride] = 8.0
    seed = np.tile(np.asarray(MAX_DRAW_SEEDS, np.uint64), per_seed)
    lam = np.exp(raw[:, 0::stride].astype(np.float64)).astype(np.float32)
    total = np.zeros(n, np.float32)
    for k in range(8):
        total = total + lam[:, k]
    weight = lam / total[:, None]
    u, missed = np.full(n, U_MAX, np.float32), np.ones(n, bool)
    for k in range(8):
        caught = missed & (u < weight[:, k])
        missed &= ~caught
        u = np.where(missed, u - weight[:, k], u)
    mu = raw.reshape(n, 8, stride)[:, :, 2:]
    return raw, seed, missed, _unit(mu)


def test_the_max_draw_seeds_are_what_they_are_said_to_be(oracle):
    assert (_first_draw_bits(np.asarray(MAX_DRAW_SEEDS, np.uint64)) == 0x7fffff).all()
    for s in MAX_DRAW_SEEDS:
        assert oracle.pcg_float(oracle.pcg_seed(s, 1)) == float(U_MAX)
    # and the search that found them, over a sixteenth of its range
    seed = np.arange(24 << 20, 28 << 20, dtype=np.uint64)
    assert [int(s) for s in seed[_first_draw_bits(seed) == 0x7fffff]] == [26240590]


@pytest.mark.parametrize("dims", [2, 3])
def test_the_oracle_falls_back_to_lobe_0(oracle, dims):
    """distribution.h:186-198 / :333-345 return lobe 0's sample when the loop ends without a pick.  The restatement uses numpy's
    exp, not the oracle's, so a row at the very edge may be told wrongly: at least 4 rows (3 % of 2 100 are expected) must be
    told to fall through AND be sampled about lobe 0's mean, and about no other lobe's; every other row is caught by the last lobe
    at the latest, and almost all by the last"""
    raw, seed, missed, mu = _fall_through_batch(dims)
    name = "vmm_pdf_sample" if dims == 2 else "vmm3_pdf_sample"
    _, d = getattr(oracle, name)(raw, np.zeros((len(raw), dims), np.float32), seed)
    cos = (mu * d[:, None, :]).sum(2)
    about = cos > 0.995
    lobe0 = missed & about[:, 0] & (about.sum(1) == 1)
    print(dims, int(missed.sum()), int(lobe0.sum()), int((~missed & about[:, 7]).sum()))
    assert missed.sum() >= 4 and lobe0.sum() >= 4
    assert (~missed & about[:, 7]).sum() > 0.9 * (~missed).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [2, 3])
def test_hip_pick_falls_back_to_lobe_0_like_the_oracle(oracle, dims):
    raw, seed, missed, _ = _fall_through_batch(dims)
    assert missed.sum() >= 4
    pdf_sample, _, dev = _mixture_calls(dims)
    wi = np.zeros((len(raw), dims), np.float32)
    rp, rd = getattr(oracle, pdf_sample)(raw, wi, seed)
    gp, gd = getattr(dev, pdf_sample)(raw, wi, seed)
    assert np.array_equal(gp, rp) and np.array_equal(gd, rd), np.flatnonzero((gd != rd).any(1))[:8]
