"""Guided integrator (BASELINE configs 4-5).

The reference's guided result is not bit-reproducible (atomic-ordered training set, fp16
network, tiny-cuda-nn absent => PARITY UNPINNED).  What is checked here:
  CPU: the oracle (oracle/wost_guided.c) is deterministic, unbiased against an analytic Laplace
       solution with mixed boundaries, and its training records obey the reference's rules;
  GPU: the HIP integrator (elaina_amd/csrc/wost_guided.hip) against the oracle -- bit-exact
       in every regime (unguided depths, a frozen network, the records of the first training
       pass, full training): both sides use the same deterministic exp/log/sin/cos and
       fp64 cos/acos/log kernels and the same k-ordered fmaf chains in the
       network; gradients are summed in 64-bit fixed point with integer atomics, so training is
       order-independent as well and a whole trained solve equals the oracle's bit for bit.
"""
import os

import numpy as np
import pytest

from conftest import box_problem
from oracle.oracle import default_net_config, guided_settings

AABB = ((-0.1, -0.1), (1.1, 1.1))
EPS = 1e-3


def laplace_box():
    # u(x, y) = y on the unit square: Dirichlet bottom/top, zero-flux Neumann left/right
    return box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.0, n_per_side=8)


def eval_ys(prob, w, h):
    s, cx, cy, ux, uy = [float(v) for v in prob.probe]
    py = (np.arange(h) * 2.0 / h - 1.0)[:, None] * np.ones((1, w))
    px = (np.arange(w) * 2.0 / w - 1.0)[None, :] * np.ones((h, 1))
    # u = (up.y, -up.x), v = up  (core/evaluation_grid.h:27-33)
    return (s * (px * (-ux) + py * uy) + cy).astype(np.float32)


def init_params(oracle, cfg, seed):
    rng = np.random.default_rng(seed)
    n = oracle.net_n_params(cfg)
    p = np.zeros(n, np.float32)
    off = 0
    for no, ni in [(64, 32), (64, 64), (64, 64), (48, 64)]:
        s = np.sqrt(6.0 / (ni + no))
        p[off:off + no * ni] = rng.uniform(-s, s, no * ni)
        off += no * ni
    p[off:] = rng.uniform(-1e-4, 1e-4, n - off)
    return p


def test_oracle_guided_is_deterministic_and_unbiased(oracle):
    cfg = default_net_config()
    prob = laplace_box()
    w = h = 20
    gs = guided_settings(w, h, 48, 48, EPS, AABB[0], AABB[1], train_spp_count=24, batch_size=1024, min_batch_size=256)
    p1, p2 = init_params(oracle, cfg, 1), init_params(oracle, cfg, 1)
    r1 = oracle.solve_guided(prob.as_dict(), gs, cfg, p1, threads=8)
    r2 = oracle.solve_guided(prob.as_dict(), gs, cfg, p2, threads=3)
    assert np.array_equal(r1["field"], r2["field"]) and np.array_equal(p1, p2)      # thread count must not matter
    assert r1["optimizer_steps"] > 0 and r1["guided_steps"] > 0
    assert r1["walks_started"] == w * h * 48
    assert r1["walks_absorbed"] + r1["walks_truncated"] == r1["walks_started"]
    ys = eval_ys(prob, w, h)
    f = r1["field"][:, 0].reshape(h, w)
    # per pixel sigma <= 0.5 / sqrt(48); the mean over 400 pixels is ~20x tighter; truncation bias < 1 %
    assert abs(float(np.mean(f - ys))) < 0.02
    assert float(np.sqrt(np.mean((f - ys) ** 2))) < 0.12
    assert np.array_equal(r1["field"][:, 0], r1["field"][:, 1])


def test_oracle_training_records_follow_reference_rules(oracle):
    cfg = default_net_config()
    prob = laplace_box()
    w = h = 16
    gs = guided_settings(w, h, 1, 32, EPS, AABB[0], AABB[1], train_spp_count=1, min_batch_size=10 ** 9)
    p = init_params(oracle, cfg, 2)
    p0 = p.copy()
    r = oracle.solve_guided(prob.as_dict(), gs, cfg, p, threads=4, dump_spp=0)
    ts = r["train_set"]
    n = len(ts["xy"])
    assert r["optimizer_steps"] == 0 and np.array_equal(p, p0)      # batch below the minimum: no step
    assert 0 < n <= 3 * w * h and n == r["train_samples"]            # maxTrainDepth = 3 records per walk
    assert np.all(ts["xy"] > 0) and np.all(ts["xy"] < 1)
    np.testing.assert_allclose(np.linalg.norm(ts["dir"], axis=1), 1.0, atol=1e-5)
    assert np.all(ts["dir_pdf"] > 0) and np.all(ts["solution"] >= 0)
    # freshly initialised mixture (kappa ~ e^+-1): the MIS pdf stays within a small factor of the
    # uniform density, 1/2pi in the interior and 1/pi on the Neumann boundary
    expect = np.where(ts["on_neumann"] != 0, 1 / np.pi, 1 / (2 * np.pi))
    assert np.all(ts["dir_pdf"] > expect / 3) and np.all(ts["dir_pdf"] < expect * 3)
    # first record of every walk starts at the evaluation point, off the boundary
    assert ts["on_neumann"][0] == 0
    # stride 2 halves the training pixels
    gs2 = guided_settings(w, h, 1, 32, EPS, AABB[0], AABB[1], train_spp_count=1, min_batch_size=10 ** 9,
                          train_pixel_stride=2, train_pixel_offset=1)
    r2 = oracle.solve_guided(prob.as_dict(), gs2, cfg, p0.copy(), threads=4, dump_spp=0)
    assert 0.3 * n < r2["train_samples"] < 0.7 * n
    assert np.array_equal(r2["field"], r["field"])                    # records never change the walk


def test_oracle_guided_phase_switch_and_quirks(oracle):
    cfg = default_net_config()
    prob = laplace_box()
    w = h = 12
    base = dict(train_spp_count=0, min_batch_size=10 ** 9)
    # max guided depth 0 in both phases: plain uniform walks, no mixture step at all
    g0 = guided_settings(w, h, 4, 32, EPS, AABB[0], AABB[1], max_guided_depth=(0, 0), **base)
    r0 = oracle.solve_guided(prob.as_dict(), g0, cfg, init_params(oracle, cfg, 3), threads=4)
    assert r0["guided_steps"] == 0
    # uniform fraction 0: every in-box step is guided (no routing draw)
    g1 = guided_settings(w, h, 4, 32, EPS, AABB[0], AABB[1], uniform_fraction=(0.0, 0.0), **base)
    r1 = oracle.solve_guided(prob.as_dict(), g1, cfg, init_params(oracle, cfg, 3), threads=4)
    assert r1["guided_steps"] > 0.5 * r1["walk_steps"]
    # uniform fraction 1: the guided kernel is never launched, walks routed to it end (reference :1031)
    g2 = guided_settings(w, h, 4, 32, EPS, AABB[0], AABB[1], uniform_fraction=(1.0, 1.0), **base)
    r2 = oracle.solve_guided(prob.as_dict(), g2, cfg, init_params(oracle, cfg, 3), threads=4)
    assert r2["guided_steps"] == 0
    assert r2["walks_absorbed"] + r2["walks_truncated"] < r2["walks_started"]
    # a box that excludes the domain disables guiding everywhere
    g3 = guided_settings(w, h, 4, 32, EPS, (5.0, 5.0), (6.0, 6.0), **base)
    r3 = oracle.solve_guided(prob.as_dict(), g3, cfg, init_params(oracle, cfg, 3), threads=4)
    assert r3["guided_steps"] == 0 and r3["walks_absorbed"] + r3["walks_truncated"] == r3["walks_started"]


# ---- HIP integrator against the oracle ---------------------------------------------------------
def _gpu_and_oracle(oracle, prob, w, h, spp, depth, train_spp, uf=(0.5, 0.5), mgd=(10, 10), batch=2048, min_batch=512,
                    params=None, seed=7, dump=True, stride=1, offset=0, aabb=None, cfg=None, ref=None):
    """cfg: the oracle's NetConfig of another network shape (default: the reference's); ref["params"]: the oracle's weights after the solve;
    ref: the oracle's half of this solve where it has been computed already"""
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    network_config = None
    if cfg is not None:
        from elaina_amd import capi
        network_config = capi.NetConfig(cfg.n_levels, cfg.n_features, cfg.base_resolution, cfg.per_level_scale, cfg.n_neurons, cfg.n_hidden_layers,
                                        cfg.n_output, cfg.learning_rate, cfg.beta1, cfg.beta2, cfg.epsilon, cfg.l2_reg, cfg.ema_decay)
    cfg = cfg or default_net_config()
    aabb = aabb or AABB
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=train_spp, maxWalkingDepth=depth,
                                  epsilonShell=EPS, uniformFractionInTrainingPhase=uf[0],
                                  uniformFractionInGuidingPhase=uf[1], maxGuidedDepthInTrainingPhase=mgd[0],
                                  maxGuidedDepthInGuidingPhase=mgd[1], batchSize=batch, minBatchSize=min_batch,
                                  trainPixelStride=stride, trainPixelOffset=offset)
    gi = GuidedIntegrator(prob, st, aabb, network_config=network_config, seed=seed)
    if params is not None:
        gi.network.set_params(params)
    p0 = gi.network.params()
    gi.solve()
    if ref is not None:
        return gi, ref
    gs = guided_settings(w, h, spp, depth, EPS, aabb[0], aabb[1], train_spp_count=train_spp, uniform_fraction=uf,
                         max_guided_depth=mgd, batch_size=batch, min_batch_size=min_batch, train_pixel_stride=stride,
                         train_pixel_offset=offset)
    dump_spp = min(train_spp, spp) - 1 if (dump and train_spp > 0) else -1
    trained = p0.copy()
    ref = oracle.solve_guided(prob.as_dict(), gs, cfg, trained, threads=16, dump_spp=dump_spp)
    ref["params"] = trained
    return gi, ref


def _close_fraction(a, b, rtol=1e-4, floor=1e-3):
    return float(np.mean(np.abs(a - b) <= rtol * np.maximum(np.abs(b), floor)))


@pytest.mark.gpu
def test_gpu_unguided_depths_are_bit_exact(oracle):
    """max guided depth 0: separate / Neumann sampling / oneStepWalk of the guided integrator
    (R_B without the 0.99 factor), no mixture arithmetic -> bit-exact like the uniform path"""
    prob = laplace_box()
    gi, ref = _gpu_and_oracle(oracle, prob, 40, 33, 4, 32, 0, mgd=(0, 0))
    assert np.array_equal(gi.solution, ref["field"])
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps"):
        assert gi.last_stats[k] == ref[k], k
    gi.close()


@pytest.mark.gpu
def test_gpu_first_pass_records_match_oracle(oracle):
    """one training pass without an optimizer step: routing, mixture sampling, MIS pdf, records and
    the ordered training set, bit for bit"""
    prob = laplace_box()
    gi, ref = _gpu_and_oracle(oracle, prob, 48, 48, 1, 32, 1, min_batch=10 ** 9)
    ts, to = gi.train_set(), ref["train_set"]
    assert gi.last_stats["optimizer_steps"] == 0
    assert gi.last_stats["train_samples"] == len(ts["xy"]) == len(to["xy"]) == ref["train_samples"]
    assert np.array_equal(gi.solution, ref["field"])
    for k in ("xy", "dir", "solution", "dir_pdf", "normal", "on_neumann"):
        assert np.array_equal(ts[k], to[k]), k
    for k in ("walk_steps", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps"):
        assert gi.last_stats[k] == ref[k], k
    gi.close()


def _check_first_pass(gi, ref):
    """the assertions of test_gpu_first_pass_records_match_oracle; returns the size of the training set"""
    ts, to = gi.train_set(), ref["train_set"]
    assert gi.last_stats["optimizer_steps"] == 0
    assert gi.last_stats["train_samples"] == len(ts["xy"]) == len(to["xy"]) == ref["train_samples"]
    assert np.array_equal(gi.solution, ref["field"])
    for k in ("xy", "dir", "solution", "dir_pdf", "normal", "on_neumann"):
        assert np.array_equal(ts[k], to[k]), k
    for k in ("walk_steps", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps"):
        assert gi.last_stats[k] == ref[k], k
    return len(ts["xy"])


@pytest.mark.gpu
def test_gpu_first_pass_records_past_one_scan_chunk(oracle):
    """258 blocks of 256 training pixels: the scan of the block sums (256 threads) takes a second trip with the carry of the
    first -- records and the ordered training set bit for bit"""
    prob = laplace_box()
    w, h = 258, 256
    assert (w * h + 255) // 256 > 256
    gi, ref = _gpu_and_oracle(oracle, prob, w, h, 1, 8, 1, min_batch=10 ** 9)
    _check_first_pass(gi, ref)
    gi.close()


@pytest.mark.gpu
def test_gpu_first_pass_records_rejected_by_the_box(oracle):
    """a guiding box inside the domain: records outside it are written by the walk and left out of the training set, so a
    pixel's count and its depth differ -- bit for bit; fewer entries than with the box around the domain"""
    prob = laplace_box()
    aabb = ((0.25, 0.2), (0.8, 0.7))
    gi, ref = _gpu_and_oracle(oracle, prob, 48, 48, 1, 32, 1, min_batch=10 ** 9, aabb=aabb)
    n = _check_first_pass(gi, ref)
    gs = guided_settings(48, 48, 1, 32, EPS, AABB[0], AABB[1], train_spp_count=1, min_batch_size=10 ** 9)
    usual = oracle.solve_guided(prob.as_dict(), gs, default_net_config(), gi.network.params(), threads=16)["train_samples"]
    assert 0 < n < usual
    gi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("spp,uf", [(8, (0.5, 0.5)), (3, (0.0, 0.0)), (3, (0.9, 0.25))])
def test_gpu_frozen_network_matches_oracle(oracle, spp, uf):
    """training off, a random network with mild lobes (MLP weights in +-0.3: raw outputs in [-2.70, 2.20] and log kappa <= 1.82,
    so kappa <= 6.2, no end of the clamp is touched and 0.03 % of the lobes reach log_bessel's branch from kappa 3.75;
    test_guided_saturated.py asserts these figures and holds the saturated networks): routing, mixture sampling (fp64 rejection), MIS pdf, reflection on the Neumann boundary,
    throughput -- bit-exact"""
    prob = laplace_box()
    cfg = default_net_config()
    rng = np.random.default_rng(3)
    n = oracle.net_n_params(cfg)
    p = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    p[13312:] = rng.uniform(-1, 1, n - 13312).astype(np.float32)
    gi, ref = _gpu_and_oracle(oracle, prob, 48, 40, spp, 32, 0, params=p, uf=uf)
    assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps"):
        assert gi.last_stats[k] == ref[k], k
    assert ref["guided_steps"] > 0
    assert np.array_equal(gi.network.params(), p)            # no training happened
    gi.close()


@pytest.mark.gpu
def test_gpu_frozen_network_on_ladybug_matches_oracle(oracle, ladybug):
    """the shipped scene (61 476 Dirichlet segments, Neumann box), guided walks with the freshly
    initialised network, no training: bit-exact against the oracle"""
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    w, h, spp, depth = 40, 32, 2, 48
    aabb = ((-100.0, -100.0), (600.0, 600.0))
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=0, maxWalkingDepth=depth,
                                  epsilonShell=1.0)
    gi = GuidedIntegrator(ladybug, st, aabb, seed=11)
    p0 = gi.network.params()
    gi.solve()
    gs = guided_settings(w, h, spp, depth, 1.0, aabb[0], aabb[1], train_spp_count=0)
    ref = oracle.solve_guided(ladybug.as_dict(), gs, default_net_config(), p0.copy(), threads=16)
    assert np.array_equal(gi.solution, ref["field"])
    assert gi.last_stats["walk_steps"] == ref["walk_steps"] and gi.last_stats["guided_steps"] == ref["guided_steps"] > 0
    gi.close()


@pytest.mark.gpu
def test_gpu_uniform_fraction_edge_cases(oracle):
    prob = laplace_box()
    gi, ref = _gpu_and_oracle(oracle, prob, 32, 32, 2, 32, 0, uf=(0.0, 0.0))
    assert gi.last_stats["guided_steps"] == ref["guided_steps"] and np.array_equal(gi.solution, ref["field"])
    assert gi.last_stats["guided_steps"] > 0.5 * gi.last_stats["walk_steps"]
    gi.close()
    gi, ref = _gpu_and_oracle(oracle, prob, 32, 32, 2, 32, 0, uf=(1.0, 1.0))
    assert gi.last_stats["guided_steps"] == 0 == ref["guided_steps"]
    # walks routed to the never-launched guided kernel end there, on both sides alike
    assert gi.last_stats["walks_absorbed"] + gi.last_stats["walks_truncated"] < gi.last_stats["walks_started"]
    assert gi.last_stats["walk_steps"] == ref["walk_steps"] and np.array_equal(gi.solution, ref["field"])
    gi.close()


@pytest.mark.gpu
def test_gpu_training_end_to_end_matches_oracle(oracle):
    """16 trained samples + 16 guided ones: every walk, record, batch, gradient and Adam step equal
    to the oracle's bit for bit, and the estimate unbiased against the analytic solution"""
    prob = laplace_box()
    w = h = 48
    gi, ref = _gpu_and_oracle(oracle, prob, w, h, 32, 32, 16, dump=False)
    st = gi.last_stats
    assert st["optimizer_steps"] == ref["optimizer_steps"] > 0
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps",
              "train_samples"):
        assert st[k] == ref[k], k
    assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
    assert st["walks_absorbed"] + st["walks_truncated"] == st["walks_started"] == w * h * 32
    ys = eval_ys(prob, w, h)
    f = gi.solution[:, 0].reshape(h, w)
    assert abs(float(np.mean(f - ys))) < 0.02 and float(np.sqrt(np.mean((f - ys) ** 2))) < 0.15
    assert np.array_equal(gi.solution[:, 0], gi.solution[:, 2])
    # the trained network moved away from its initialisation, EMA weights follow
    assert np.abs(gi.network.params() - gi.network.inference_params()).max() > 0
    gi.close()


@pytest.mark.gpu
def test_gpu_training_end_to_end_with_scalar_network_kernels(oracle, monkeypatch):
    """the same solve through the one-thread-per-point network kernels (WOST_NET_SCALAR=1)"""
    monkeypatch.setenv("WOST_NET_SCALAR", "1")
    prob = laplace_box()
    gi, ref = _gpu_and_oracle(oracle, prob, 32, 32, 6, 32, 4, dump=False)
    assert gi.last_stats["optimizer_steps"] == ref["optimizer_steps"] > 0
    assert np.array_equal(gi.solution, ref["field"])
    gi.close()


@pytest.mark.gpu
def test_gpu_trained_solve_is_reproducible(oracle):
    """two runs of the same trained solve give the same field and the same network"""
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    out = []
    for _ in range(2):
        st = GuidedIntegratorSettings(frameSize=(64, 64), samplesPerPixel=12, trainSppCount=8, maxWalkingDepth=32,
                                      epsilonShell=EPS, batchSize=4096, minBatchSize=1024)
        gi = GuidedIntegrator(prob, st, AABB, seed=5)
        gi.solve()
        assert gi.last_stats["optimizer_steps"] > 0
        out.append((gi.solution.copy(), gi.network.params()))
        gi.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_gpu_training_pixel_stride(oracle):
    prob = laplace_box()
    gi, ref = _gpu_and_oracle(oracle, prob, 32, 32, 1, 32, 1, min_batch=10 ** 9, stride=3, offset=2)
    assert gi.last_stats["train_samples"] == ref["train_samples"]
    assert np.array_equal(gi.train_set()["xy"], ref["train_set"]["xy"])
    full, _ = _gpu_and_oracle(oracle, prob, 32, 32, 1, 32, 1, min_batch=10 ** 9)
    assert 0.25 * full.last_stats["train_samples"] < gi.last_stats["train_samples"] < 0.42 * full.last_stats["train_samples"]
    assert np.array_equal(full.solution, gi.solution)         # recording never changes a walk
    gi.close()
    full.close()


@pytest.mark.gpu
def test_gpu_guided_on_ladybug_agrees_with_uniform(ladybug, oracle):
    """BASELINE config 4 in miniature: ladybug scene, guided integrator with online training
    against the uniform integrator (both unbiased for the same field; the guided one has no
    0.99 shrink, so only statistics can be compared)"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    w = h = 96
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=64, trainSppCount=32, maxWalkingDepth=64,
                                  epsilonShell=1.0, batchSize=8192, minBatchSize=2048)
    gi = GuidedIntegrator(ladybug, st, ((-100.0, -100.0), (600.0, 600.0)))
    gi.solve()
    ui = UniformIntegrator(ladybug, UniformIntegratorSettings(frameSize=(w, h), samplesPerPixel=1024, maxWalkingDepth=64,
                                                              epsilonShell=1.0))
    ui.solve()
    u64 = UniformIntegrator(ladybug, UniformIntegratorSettings(frameSize=(w, h), samplesPerPixel=64, maxWalkingDepth=64,
                                                               epsilonShell=1.0))
    u64.solve()
    ref = ui.solution
    rms_g = float(np.sqrt(np.mean((gi.solution - ref) ** 2)))
    rms_u = float(np.sqrt(np.mean((u64.solution - ref) ** 2)))
    assert gi.last_stats["optimizer_steps"] > 0
    assert abs(float(gi.solution.mean()) - float(ref.mean())) < 0.01 * abs(float(ref.mean())) + 1e-3
    assert rms_g < 1.5 * rms_u + 1e-3, (rms_g, rms_u)
    gi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_guiding_reduces_the_variance(precision):
    """What rows a21-a27 are FOR.  Oracle and kernels share an author, so a common error in the training target
    (|solution / thp|, train.h:423-471), in the sign of the loss or in the MIS weights that leaves the estimator unbiased
    would pass every bit-exact test; only this one can catch it.  A small bright Dirichlet disc and a large dark one in a
    reflecting box (elaina_amd/scenes.py): 64 trained + 64 guided samples must beat 128 uniform ones by a clear margin
    against a 8192-sample field of the uniform integrator (measured: 0.71 of the uniform RMSE in both precisions), stay
    unbiased, and the learned mixture must point at the bright disc."""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    from elaina_amd.scenes import BRIGHT_DISC_AABB, BRIGHT_DISC_CENTRE, bright_disc_scene, mixture_mean_direction
    p = bright_disc_scene()
    w, depth, eps = 128, 128, 0.05
    it = UniformIntegrator(p, UniformIntegratorSettings((w, w), 8192, depth, eps))
    it.solve()
    ref = it.solution.copy()
    it.close()
    it = UniformIntegrator(p, UniformIntegratorSettings((w, w), 128, depth, eps))
    it.solve()
    rmse_u = float(np.sqrt(np.mean((it.solution - ref) ** 2)))
    it.close()
    st = GuidedIntegratorSettings(frameSize=(w, w), samplesPerPixel=128, trainSppCount=64, maxWalkingDepth=depth, epsilonShell=eps,
                                  uniformFractionInTrainingPhase=0.5, uniformFractionInGuidingPhase=0.5,       # data/ladybug/n.json
                                  batchSize=65536, minBatchSize=8192)
    g = GuidedIntegrator(p, st, BRIGHT_DISC_AABB)
    if precision == 16:
        g.network.set_option("precision", 16)
        g.network.set_option("train_precision", 16)
    g.solve()
    rmse_g = float(np.sqrt(np.mean((g.solution - ref) ** 2)))
    assert g.last_stats["optimizer_steps"] > 0 and g.last_stats["guided_steps"] > 0.2 * g.last_stats["walk_steps"]
    assert rmse_g <= 0.8 * rmse_u, (rmse_g, rmse_u)
    assert abs(float(g.solution.mean()) - float(ref.mean())) < 0.01 * float(ref.mean())
    # the mixture at the centre of the box: its mean direction is the direction of the bright disc
    q = np.asarray((50.0, 50.0), np.float32)
    mean_dir = mixture_mean_direction(g.queryNetwork(q))
    to_bright = np.asarray(BRIGHT_DISC_CENTRE) - q
    cos = float(mean_dir @ to_bright) / (np.linalg.norm(mean_dir) * np.linalg.norm(to_bright))
    assert cos > 0.9 and np.linalg.norm(mean_dir) > 0.05, (cos, mean_dir)
    g.close()


@pytest.mark.gpu
def test_gpu_sharded_guided_solve(oracle):
    """wost_guided_solve_sharded: with a frozen network the shards sum to exactly the full-frame
    field; with training every shard fits its own network and the sum stays unbiased"""
    import torch
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    w, h = 40, 24
    cfg = default_net_config()
    p = np.random.default_rng(5).uniform(-0.3, 0.3, oracle.net_n_params(cfg)).astype(np.float32)

    def make(train_spp, spp):
        st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=train_spp, maxWalkingDepth=32,
                                      epsilonShell=EPS, batchSize=1024, minBatchSize=256)
        gi = GuidedIntegrator(prob, st, AABB, seed=3)
        gi.network.set_params(p)
        return gi

    full = make(0, 4)
    full.solve()
    total = torch.zeros(w * h * 3, device="cuda")
    steps = 0
    for r in range(3):
        gi = make(0, 4)
        buf = torch.full((w * h * 3,), 7.0, device="cuda")      # must be overwritten, other shards' pixels with 0
        st = gi.solve_sharded(r, 3, buf.data_ptr())
        torch.cuda.synchronize()
        total += buf
        steps += st["walk_steps"]
        gi.close()
    assert np.array_equal(total.cpu().numpy().reshape(-1, 3), full.solution)
    assert steps == full.last_stats["walk_steps"]
    full.close()
    # with training: each shard trains on its own records
    total = torch.zeros(w * h * 3, device="cuda")
    opt = 0
    for r in range(2):
        gi = make(8, 16)
        buf = torch.zeros(w * h * 3, device="cuda")
        st = gi.solve_sharded(r, 2, buf.data_ptr())
        torch.cuda.synchronize()
        total += buf
        opt += st["optimizer_steps"]
        gi.close()
    assert opt > 0
    ys = eval_ys(prob, w, h)
    f = total.cpu().numpy().reshape(-1, 3)[:, 0].reshape(h, w)
    assert abs(float(np.mean(f - ys))) < 0.03


@pytest.mark.gpu
def test_gpu_guided_with_source_term_matches_oracle(oracle):
    """guided integrator on a Poisson problem (sampleSource + recordSourceContribution), frozen and
    trained: bit-exact, and unbiased against u = (1 - r^2) / 4"""
    from test_oracle_solver import _poisson_disc
    prob = _poisson_disc()
    gi, ref = _gpu_and_oracle(oracle, prob, 40, 40, 24, 48, 12, batch=2048, min_batch=512, dump=False,
                              aabb=((-1.2, -1.2), (1.2, 1.2)))
    assert gi.last_stats["optimizer_steps"] == ref["optimizer_steps"] > 0
    assert np.array_equal(gi.solution, ref["field"])
    ys, xs = np.mgrid[0:40, 0:40]
    x, y = (xs * 2 / 40 - 1) * 0.7, (ys * 2 / 40 - 1) * 0.7
    want = (1 - x ** 2 - y ** 2) / 4
    f = gi.solution[:, 0].reshape(40, 40)
    assert abs(float(np.mean(f - want))) < 5e-3
    gi.close()


def _exact(gi, ref):
    assert np.array_equal(gi.solution, ref["field"]), float(np.abs(gi.solution - ref["field"]).max())
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps",
              "train_samples", "optimizer_steps"):
        assert gi.last_stats[k] == ref[k], k


@pytest.mark.gpu
def test_gpu_guided_edge_cases_match_oracle(oracle):
    """the instantiations and corner cases the shipped scenes never reach: a 3000-segment emissive
    Neumann boundary (tree queries, SNCH cones), Dirichlet only, a masked ragged frame, depth 1,
    training longer than the solve, zero samples"""
    from conftest import wiggly_problem
    big = ((-140.0, -140.0), (140.0, 140.0))
    gi, ref = _gpu_and_oracle(oracle, wiggly_problem(emissive=True), 36, 28, 6, 40, 3, batch=1024, min_batch=256,
                              aabb=big, dump=False)
    _exact(gi, ref)
    assert ref["neumann_hits"] > 0 and ref["optimizer_steps"] > 0
    gi.close()
    # open Neumann polyline (silhouette vertices at the ends), frozen network
    gi, ref = _gpu_and_oracle(oracle, wiggly_problem(open_gap=40), 30, 30, 3, 32, 0, aabb=big, dump=False)
    _exact(gi, ref)
    gi.close()
    # Dirichlet only
    prob = box_problem(value=lambda x, y: x * y)
    gi, ref = _gpu_and_oracle(oracle, prob, 33, 21, 5, 32, 2, batch=1024, min_batch=256, dump=False)
    _exact(gi, ref)
    assert ref["neumann_hits"] == 0
    gi.close()
    # mask + ragged frame + training pixel stride
    prob = laplace_box()
    prob.mask = (np.arange(37 * 19) % 5 != 0).astype(np.uint8)
    gi, ref = _gpu_and_oracle(oracle, prob, 37, 19, 6, 32, 4, batch=512, min_batch=128, stride=2, offset=1, dump=False)
    _exact(gi, ref)
    assert np.all(gi.solution[prob.mask == 0] == 0)
    gi.close()
    prob.mask = None
    # one step per walk; training longer than the solve; guided depth beyond the walk depth
    gi, ref = _gpu_and_oracle(oracle, prob, 24, 24, 3, 1, 10, batch=512, min_batch=128, dump=False)
    _exact(gi, ref)
    assert ref["walks_truncated"] > 0
    gi.close()
    gi, ref = _gpu_and_oracle(oracle, prob, 24, 24, 2, 6, 1, mgd=(50, 50), batch=512, min_batch=128, dump=False)
    _exact(gi, ref)
    gi.close()
    # guiding only in the second phase, and no samples at all
    gi, ref = _gpu_and_oracle(oracle, prob, 24, 24, 6, 24, 3, mgd=(0, 10), uf=(0.5, 0.0), batch=512, min_batch=128, dump=False)
    _exact(gi, ref)
    gi.close()
    gi, ref = _gpu_and_oracle(oracle, prob, 16, 16, 0, 8, 0, dump=False)
    assert gi.last_stats["walk_steps"] == 0 == ref["walk_steps"]
    gi.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_gpu_two_ranks_guided_runner(shared):
    """config 5 in miniature through tools/gpu_guided_bench.py with two processes on the one GPU of
    the test box (gloo carries the collectives): per-shard networks by default, ONE network --
    bit-identical on both ranks thanks to the integer gradient sums -- with --shared-network"""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tools", "gpu_guided_bench.py"), "--backend", "gloo", "--frame", "192",
           "--spp", "6", "--train-spp", "4", "--batch", "8192", "--min-batch", "2048"] + (["--shared-network"] if shared else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["n_gpus"] == 2 and r["optimizer_steps_all_ranks"] > 0 and r["shared_network"] == shared
    assert r["networks_identical"] == shared
    assert 0.4 < r["mean"] < 0.6


@pytest.mark.gpu
def test_gpu_full_frame_guided_properties(ladybug):
    """BASELINE config 4's frame (1024^2, full batch sizes) at 12 samples: reproducible with training,
    every walk accounted for, exact linearity in a power-of-two intensity while the network is
    frozen, and agreement of the mean with the uniform integrator"""
    import copy
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    aabb = ((-100.0, -100.0), (600.0, 600.0))

    def run(problem, train):
        st = GuidedIntegratorSettings(frameSize=(1024, 1024), samplesPerPixel=12, trainSppCount=train, maxWalkingDepth=64,
                                      epsilonShell=1.0)
        gi = GuidedIntegrator(problem, st, aabb, seed=42)
        gi.solve()
        out = gi.solution.copy(), dict(gi.last_stats), gi.network.params()
        gi.close()
        return out

    f1, s1, p1 = run(ladybug, 8)
    f2, s2, p2 = run(ladybug, 8)
    assert np.array_equal(f1, f2) and np.array_equal(p1, p2)
    assert s1["optimizer_steps"] == 8 * 5 and s1["walks_absorbed"] + s1["walks_truncated"] == s1["walks_started"] == 12 * 1024 * 1024
    frozen, _, _ = run(ladybug, 0)
    dbl = copy.copy(ladybug)
    dbl.dirichlet_intensity = 2.0
    frozen2, _, _ = run(dbl, 0)
    assert np.array_equal(frozen2, 2.0 * frozen)
    ui = UniformIntegrator(ladybug, UniformIntegratorSettings((1024, 1024), 12, 64, 1.0))
    ui.solve()
    assert abs(float(f1.mean()) - float(ui.solution.mean())) < 2e-3 * float(ui.solution.mean())
    ui.close()


# the walk steps of BASELINE config 4 at its real size: deterministic arithmetic makes the count a known answer per precision
CONFIG4_WALK_STEPS = {32: 1_892_816_878, 16: 1_892_874_274}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_config4_at_full_size(ladybug, precision):
    """BASELINE config 4 as it is benchmarked -- ladybug, 1024^2, 256 samples, all of them trained, the reference's batch sizes --
    under pytest, not only in bench.py: the walk-step count is a known answer (every walk, record, batch and Adam step is
    deterministic: fp32 bit-exact against the oracle on smaller frames, the half-precision mode reproducible), two solves give the
    same field and the same network, every walk is accounted for, 256 x 5 Adam steps were taken, and the field agrees with the
    uniform integrator's (bit-exact against the oracle) up to the Monte-Carlo noise of 256 samples"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    aabb = ((-100.0, -100.0), (600.0, 600.0))
    n = 1024 * 1024

    def run():
        st = GuidedIntegratorSettings(frameSize=(1024, 1024), samplesPerPixel=256, trainSppCount=256, maxWalkingDepth=64, epsilonShell=1.0)
        gi = GuidedIntegrator(ladybug, st, aabb)
        if precision == 16:
            gi.network.set_option("precision", 16)
            gi.network.set_option("train_precision", 16)
        gi.solve()
        out = gi.solution.copy(), dict(gi.last_stats), gi.network.params()
        gi.close()
        return out

    f1, s1, p1 = run()
    f2, s2, p2 = run()
    # strict in both precisions again (round 5): the half-precision mode's run-to-run difference -- one solve in 20 to 36 -- was the
    # training forward's first tile after a light kernel (EXPERIMENTS 20); 55 of 55 full-size pairs on two boxes agree since that is recomputed
    assert np.array_equal(f1, f2) and np.array_equal(p1, p2) and s1["walk_steps"] == s2["walk_steps"]
    assert s1["walk_steps"] == CONFIG4_WALK_STEPS[precision]
    assert s1["walks_started"] == 256 * n and s1["walks_absorbed"] + s1["walks_truncated"] == s1["walks_started"]
    assert s1["optimizer_steps"] == 256 * 5 and s1["guided_steps"] > 0.5 * s1["walk_steps"]
    assert np.isfinite(f1).all()
    ui = UniformIntegrator(ladybug, UniformIntegratorSettings((1024, 1024), 256, 64, 1.0))
    ui.solve()
    u = ui.solution
    assert abs(float(f1.mean()) - float(u.mean())) < 1e-3 * float(u.mean())
    rel = float(np.linalg.norm(f1 - u) / np.linalg.norm(u))
    assert rel < 0.05, rel          # two independent 256-sample estimates of one field (measured 0.035)
    ui.close()


@pytest.mark.gpu
def test_gpu_half_precision_training_kernels_repeat_themselves_at_full_size():
    """WOST_NET_CHECK3=1: every half-precision training kernel of every Adam step launched three times on the same inputs, the three
    results compared word by word on the device -- config 4's frame and batch size, 32 samples = 160 steps.  The guard of the
    first-tile recomputation in net_forward_h_kernel (EXPERIMENTS 20): without it the first of the three forward launches differs in
    about one step of fifty (a whole 16-point unit of a wave's first tile), which is what made one half-precision solve in twenty differ
    from the next."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ, WOST_NET_CHECK3="1", SPP="32", REPS="1")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "probes", "check3_cfg4.py")], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stderr.splitlines() if l.startswith("CHECK3 after")]
    assert lines, out.stderr[-2000:]
    assert "after 160 training steps: forward words differing 0 " in lines[-1] and "train kernel words differing 0 " in lines[-1], lines[-1]


# ---- BASELINE config 5: the 2048 x 2048 frame, one shard of 8 ---------------------------------------
def _band_of_shard_mask(w, h, rows, shard, shards):
    """mask that keeps only the pixels of `rows` evaluation rows around the middle which shard
    `shard` of `shards` owns (8x8 pixel tiles dealt round-robin)"""
    from elaina_amd.distributed import owned_mask
    m = np.zeros(w * h, np.uint8)
    b = (h // 2 - rows // 2) * w
    m[b:b + rows * w] = 1
    m &= owned_mask(w, h, shard, shards).astype(np.uint8)
    return m, b, b + rows * w


@pytest.mark.gpu
def test_gpu_config5_frame_shard_frozen_network_band_matches_oracle(oracle, ladybug):
    """The frame of BASELINE config 5 (2048^2: four times the reference's fixed 1024^2 default mask,
    core/problem.cu:245-247, and its MAX_RESOLUTION, guided/parameters.h:8) -- shard 0 of 8 of a
    guided solve with the freshly initialised network and no training.  With a frozen network a
    pixel does not depend on any other pixel, so the oracle walks only an 8-row band of the shard
    (same frame, a mask selects the band) and the band must agree bit for bit; the default mask
    (none) is sized to the frame: every owned pixel of the shard is walked."""
    from elaina_amd.distributed import owned_mask
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    import torch
    w = h = 2048
    spp, depth = 8, 64
    aabb = ((-100.0, -100.0), (600.0, 600.0))
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=0, maxWalkingDepth=depth, epsilonShell=1.0)
    gi = GuidedIntegrator(ladybug, st, aabb, seed=5)
    p0 = gi.network.params()
    field = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    stats = gi.solve_sharded(0, 8, field.data_ptr())
    torch.cuda.synchronize()
    got = field.cpu().numpy().reshape(-1, 3)
    own = owned_mask(w, h, 0, 8)
    assert stats["walks_started"] == int(own.sum()) * spp            # the whole shard, not a 1024^2 corner
    assert not got[~own].any() and np.isfinite(got).all()
    assert stats["guided_steps"] > 0 and stats["net_points"] > 0 and stats["optimizer_steps"] == 0
    gi.close()
    mask, b, e = _band_of_shard_mask(w, h, 8, 0, 8)
    sd = ladybug.as_dict()
    sd["mask"] = mask
    gs = guided_settings(w, h, spp, depth, 1.0, aabb[0], aabb[1], train_spp_count=0)
    ref = oracle.solve_guided(sd, gs, default_net_config(), p0.copy(), threads=16)
    sel = mask.astype(bool)
    assert ref["walks_started"] == int(sel.sum()) * spp
    assert np.array_equal(got[sel], ref["field"][sel]), float(np.abs(got[sel] - ref["field"][sel]).max())


@pytest.mark.gpu
def test_gpu_config5_frame_shard_trained_solve(ladybug):
    """shard 0 of 8 of the 2048^2 frame with 8 trained + 8 guided samples: counters, reproducibility
    (same field and same network twice) and agreement with the uniform integrator on the same
    pixels within Monte-Carlo noise (the guided estimator is unbiased for any network state)"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.distributed import owned_mask
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    import torch
    w = h = 2048
    aabb = ((-100.0, -100.0), (600.0, 600.0))
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=16, trainSppCount=8, maxWalkingDepth=64, epsilonShell=1.0)
    runs = []
    for _ in range(2):
        gi = GuidedIntegrator(ladybug, st, aabb, seed=9)
        field = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        s = gi.solve_sharded(0, 8, field.data_ptr())
        torch.cuda.synchronize()
        runs.append((field.cpu().numpy().reshape(-1, 3), gi.network.params(), s))
        gi.close()
    (f0, p0, s0), (f1, p1, s1) = runs
    assert np.array_equal(f0, f1) and np.array_equal(p0, p1)
    own = owned_mask(w, h, 0, 8)
    n_own = int(own.sum())
    assert n_own == w * h // 8 and s0["walks_started"] == n_own * 16
    assert s0["optimizer_steps"] > 0 and s0["train_samples"] > n_own and s0["guided_steps"] > 0
    assert s0["walks_absorbed"] + s0["walks_truncated"] == s0["walks_started"]
    for k in ("walk_steps", "train_samples", "optimizer_steps", "guided_steps"):
        assert s0[k] == s1[k], k
    ui = UniformIntegrator(ladybug, UniformIntegratorSettings((w, h), 16, 64, 1.0))
    uf = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ui.solve_sharded(0, 8, uf.data_ptr())
    torch.cuda.synchronize()
    u = uf.cpu().numpy().reshape(-1, 3)
    ui.close()
    assert not f0[~own].any()
    # two unbiased 16-spp estimates of the same field: their means agree far better than their pixels
    assert abs(float(f0[own].mean()) - float(u[own].mean())) < 2e-3 * max(1.0, abs(float(u[own].mean())))
    rel = np.linalg.norm(f0[own] - u[own]) / np.linalg.norm(u[own])
    assert rel < 0.5, rel


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_config5_sample_count_with_the_phase_switch_on_a_thin_shard(ladybug, precision):
    """BASELINE config 5's own sample count -- 1024 samples per pixel, the first 256 trained, then the switch to the guiding phase
    (reference integrator/guided/integrator.cu:991-996: uniformFraction and maxGuidedDepth change, training stops) -- on its 2048^2
    frame, for shard 0 of 64 (65 536 pixels: what keeps this inside the driver's clock).  Counters across the switch, an Adam pass
    after every trained sample and none after, reproducibility (field and network twice), and agreement with the uniform
    integrator's 1024-sample solve of the same pixels within Monte-Carlo noise."""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.distributed import owned_mask
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    import torch
    w = h = 2048
    spp, trained, shards = 1024, 256, 64
    aabb = ((-100.0, -100.0), (600.0, 600.0))
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=trained, maxWalkingDepth=64, epsilonShell=1.0)
    runs = []
    for _ in range(2):
        gi = GuidedIntegrator(ladybug, st, aabb, seed=11)
        if precision == 16:
            gi.network.set_option("precision", 16)
            gi.network.set_option("train_precision", 16)
        p_init = gi.network.params()
        field = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        s = gi.solve_sharded(0, shards, field.data_ptr())
        torch.cuda.synchronize()
        runs.append((field.cpu().numpy().reshape(-1, 3), gi.network.params(), dict(s)))
        gi.close()
    (f0, p0, s0), (f1, p1, s1) = runs
    assert np.array_equal(f0, f1) and np.array_equal(p0, p1)
    assert not np.array_equal(p0, p_init)
    own = owned_mask(w, h, 0, shards)
    n_own = int(own.sum())
    assert n_own == w * h // shards and s0["walks_started"] == n_own * spp
    assert s0["walks_absorbed"] + s0["walks_truncated"] == s0["walks_started"]
    # every trained sample is followed by at least one Adam step (65 536 pixels leave at least minBatchSize records), at most five
    # (batchesPerSpp), and the 768 guiding samples by none
    assert trained <= s0["optimizer_steps"] <= 5 * trained
    assert s0["train_samples"] >= 65536 * trained and s0["guided_steps"] > 0
    for k in ("walk_steps", "train_samples", "optimizer_steps", "guided_steps", "walks_truncated"):
        assert s0[k] == s1[k], k
    assert not f0[~own].any() and np.isfinite(f0).all()
    ui = UniformIntegrator(ladybug, UniformIntegratorSettings((w, h), spp, 64, 1.0))
    uf = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    ui.solve_sharded(0, shards, uf.data_ptr())
    torch.cuda.synchronize()
    u = uf.cpu().numpy().reshape(-1, 3)
    ui.close()
    # two unbiased 1024-sample estimates of the same pixels
    assert abs(float(f0[own].mean()) - float(u[own].mean())) < 5e-4 * max(1.0, abs(float(u[own].mean())))
    rel = np.linalg.norm(f0[own] - u[own]) / np.linalg.norm(u[own])
    assert rel < 0.05, rel


@pytest.mark.gpu
def test_gpu_train_pixel_offset_is_drawn_like_the_reference(oracle):
    """trainPixelStride > 1: prepareSolve draws trainPixelOffset = get1D() * stride from the integrator's host
    sampler, seeded setSeed(42) with sequence 1 in resetNetwork (reference integrator/guided/integrator.cu:126,
    :1134, core/sampler.h:20-27); one draw per solve.  The solves equal the oracle's with those offsets."""
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    w, h, spp, depth, stride = 36, 28, 6, 32, 3
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=3, maxWalkingDepth=depth, epsilonShell=EPS,
                                  batchSize=1024, minBatchSize=128, trainPixelStride=stride)          # trainPixelOffset = -1: drawn
    rng = oracle.pcg_seed(42, 1)
    expect = [int(np.float32(oracle.pcg_float(rng)) * np.float32(stride)) for _ in range(2)]
    assert all(0 <= e < stride for e in expect)
    gi = GuidedIntegrator(prob, st, AABB, seed=7)
    p0 = gi.network.params()
    for k in range(2):
        gi.network.set_params(p0)                    # same starting network, the next draw of the host sampler
        gi.solve()
        assert gi.last_stats["reserved"] == expect[k]
        gs = guided_settings(w, h, spp, depth, EPS, AABB[0], AABB[1], train_spp_count=3, batch_size=1024, min_batch_size=128,
                             train_pixel_stride=stride, train_pixel_offset=expect[k])
        ref = oracle.solve_guided(prob.as_dict(), gs, default_net_config(), p0.copy(), threads=8)
        assert gi.last_stats["train_samples"] == ref["train_samples"] and gi.last_stats["optimizer_steps"] == ref["optimizer_steps"] > 0
        assert np.array_equal(gi.solution, ref["field"])
    gi.close()


@pytest.mark.gpu
def test_gpu_half_precision_network_mode_is_unbiased_and_no_noisier(oracle):
    """The reference evaluates its guiding network in half precision.  With precision 16 the guided walk
    samples from a slightly different (but valid, normalised) mixture: the estimator stays unbiased -- its
    field agrees with the analytic solution as well as the fp32-mode field does -- the variance is not
    worse, and the solve is reproducible bit for bit.  fp32 remains the default, bit-exact mode."""
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    w = h = 64
    spp = 48
    exact = eval_ys(prob, w, h).reshape(-1)
    fields = {}
    for prec in (32, 16, 16):
        st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=24, maxWalkingDepth=48, epsilonShell=EPS,
                                      batchSize=4096, minBatchSize=1024)
        gi = GuidedIntegrator(prob, st, AABB, seed=3)
        if prec == 16:
            gi.network.set_option("precision", 16)
        gi.solve()
        assert gi.last_stats["optimizer_steps"] > 0 and gi.last_stats["guided_steps"] > 0
        fields.setdefault(prec, []).append((gi.solution[:, 0].copy(), gi.network.params()))
        gi.close()
    f32 = fields[32][0][0]
    (h1, p1), (h2, p2) = fields[16]
    assert np.isfinite(h1).all() and np.isfinite(f32).all()
    assert np.array_equal(h1, h2) and np.array_equal(p1, p2)                 # reproducible
    assert not np.array_equal(h1, f32)                                         # a different (half-precision) sampler
    e32, e16 = f32 - exact, h1 - exact
    assert abs(float(e16.mean())) < 4e-3 and abs(float(e32.mean())) < 4e-3     # both unbiased
    r32, r16 = float(np.sqrt((e32 ** 2).mean())), float(np.sqrt((e16 ** 2).mean()))
    assert r16 < 1.15 * r32, (r16, r32)                                        # variance not worse (same spp)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("scene", ["box", "ladybug", "wiggly", "source"])
def test_gpu_fused_sample_kernel_equals_the_per_depth_launches(scene, precision, oracle, monkeypatch):
    """A whole sample runs in ONE launch: walkers stay in their lanes from depth to depth and every wave
    evaluates the network for its own walkers (guided_sample_kernel; fp32 fragments in the default mode, the
    f16 image in the half-precision mode).  Per pixel nothing changes -- same draws, same network arithmetic,
    same records -- so the field, the statistics and the trained weights equal those of the
    one-launch-per-depth path (WOST_GUIDED_FUSED=0) bit for bit.  (In the fp32 mode every other test of this
    file compares the fused path with the oracle.)"""
    from elaina_amd import Problem
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    if scene == "box":
        prob, aabb, w, h, eps, depth = laplace_box(), AABB, 64, 48, EPS, 40
    elif scene == "ladybug":
        prob, aabb, w, h, eps, depth = Problem.load_scene("ladybug"), ((-100.0, -100.0), (600.0, 600.0)), 96, 96, 1.0, 64
    elif scene == "wiggly":
        # 3000-segment emissive Neumann boundary: tree queries and Neumann sampling inside the step
        from conftest import wiggly_problem
        prob, aabb, w, h, eps, depth = wiggly_problem(emissive=True), ((-140.0, -140.0), (140.0, 140.0)), 36, 28, EPS, 40
    else:
        from test_oracle_solver import _poisson_disc
        prob, aabb, w, h, eps, depth = _poisson_disc(), ((-1.2, -1.2), (1.2, 1.2)), 40, 40, EPS, 48
    out = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("WOST_GUIDED_FUSED", fused)
        st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=10, trainSppCount=6, maxWalkingDepth=depth, epsilonShell=eps,
                                      maxGuidedDepthInTrainingPhase=5, maxGuidedDepthInGuidingPhase=7, batchSize=4096, minBatchSize=512,
                                      trainPixelStride=2)
        gi = GuidedIntegrator(prob, st, aabb, seed=11)
        if precision == 16:
            gi.network.set_option("precision", 16)
            gi.network.set_option("train_precision", 16)
        gi.solve()
        stats = dict(gi.last_stats)
        out[fused] = (gi.solution.copy(), gi.network.params(), gi.network.inference_params(), stats)
        gi.close()
    (f0, p0, i0, s0), (f1, p1, i1, s1) = out["0"], out["1"]
    assert s1["kernel_launches"] < s0["kernel_launches"]
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps", "net_points",
              "train_samples", "optimizer_steps"):
        assert s0[k] == s1[k], (k, s0[k], s1[k])
    assert s1["optimizer_steps"] > 0 and s1["guided_steps"] > 0
    assert np.isfinite(f1).all()
    assert np.array_equal(p0, p1) and np.array_equal(i0, i1)
    assert np.array_equal(f0, f1), float(np.abs(f0 - f1).max())


@pytest.mark.gpu
def test_gpu_fused_sample_kernel_edge_cases(monkeypatch):
    """the fused path against the per-depth path where the launch logic differs: a masked ragged frame (row-major
    pixel order), pixel shards, one step per walk, guiding only after the training phase, guided depth beyond
    the walk depth, no training at all (all samples in one launch), and a solve repeated on the same handle"""
    import torch
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()

    def run(fused, w, h, spp, train, depth, mgd=(5, 7), uf=(0.5, 0.5), shard=None, stride=1, twice=False):
        monkeypatch.setenv("WOST_GUIDED_FUSED", fused)
        st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=train, maxWalkingDepth=depth, epsilonShell=EPS,
                                      uniformFractionInTrainingPhase=uf[0], uniformFractionInGuidingPhase=uf[1],
                                      maxGuidedDepthInTrainingPhase=mgd[0], maxGuidedDepthInGuidingPhase=mgd[1], batchSize=1024,
                                      minBatchSize=256, trainPixelStride=stride)
        gi = GuidedIntegrator(prob, st, AABB, seed=5)
        gi.network.set_option("precision", 16)
        gi.network.set_option("train_precision", 16)
        outs = []
        for _ in range(2 if twice else 1):
            if shard is None:
                gi.solve()
                f = gi.solution.copy()
            else:
                buf = torch.full((w * h * 3,), 7.0, device="cuda")
                gi.solve_sharded(shard[0], shard[1], buf.data_ptr())
                torch.cuda.synchronize()
                f = buf.cpu().numpy().reshape(-1, 3)
            st_ = {k: v for k, v in gi.last_stats.items() if k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated",
                                                                    "neumann_hits", "guided_steps", "net_points", "train_samples")}
            outs.append((f, gi.network.params(), st_))
        gi.close()
        return outs

    cases = {
        "masked ragged frame, training pixel stride": dict(w=37, h=19, spp=6, train=4, depth=32, stride=2),
        "shard 1 of 3": dict(w=40, h=24, spp=6, train=3, depth=32, shard=(1, 3)),
        "one step per walk": dict(w=24, h=24, spp=3, train=10, depth=1),
        "guided depth beyond the walk depth": dict(w=24, h=24, spp=3, train=1, depth=6, mgd=(50, 50)),
        "guiding only in the second phase": dict(w=24, h=24, spp=6, train=3, depth=24, mgd=(0, 10), uf=(0.5, 0.0)),
        "no training: every sample in one launch": dict(w=32, h=32, spp=9, train=0, depth=40),
        "two solves on one handle": dict(w=24, h=16, spp=4, train=2, depth=24, twice=True),
    }
    for name, kw in cases.items():
        if name.startswith("masked"):
            prob.mask = (np.arange(37 * 19) % 5 != 0).astype(np.uint8)
        a, b = run("0", **kw), run("1", **kw)
        prob.mask = None
        for (f0, p0, s0), (f1, p1, s1) in zip(a, b):
            assert s0 == s1, (name, s0, s1)
            assert np.array_equal(p0, p1), name
            assert np.array_equal(f0, f1), (name, float(np.abs(f0 - f1).max()))
        if name.startswith("masked"):
            assert np.all(b[0][0][(np.arange(37 * 19) % 5) == 0] == 0)


@pytest.mark.gpu
def test_gpu_fused_sample_kernel_intermediate_frames(monkeypatch):
    """intermediate frames cut the multi-sample launches of the guiding phase at the samples the caller asked for:
    the frames (and the samples they arrive after) are those of the per-depth path"""
    import ctypes as C
    from elaina_amd import capi
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    w, h = 24, 16
    got = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("WOST_GUIDED_FUSED", fused)
        st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=14, trainSppCount=3, maxWalkingDepth=24, epsilonShell=EPS,
                                      batchSize=1024, minBatchSize=256)
        gi = GuidedIntegrator(prob, st, AABB, seed=5)
        gi.network.set_option("precision", 16)
        frames = []

        def cb(user, reason, sample, ms, field):
            frames.append((reason, sample, np.ctypeslib.as_array(field, shape=(w * h * 3,)).copy()))
            return 0

        fn = capi.FRAME_FN(cb)
        assert gi.lib.wost_guided_set_frame_callback(gi._handle, fn, None, 4, 10, 5) == 0      # spp frames at 0, 4, 8; time frames at 0, 5, 10
        gi.solve()
        got[fused] = (frames, gi.solution.copy())
        gi.close()
    (fa, sa), (fb, sb) = got["0"], got["1"]
    assert [(r, k) for r, k, _ in fa] == [(r, k) for r, k, _ in fb] == [(0, 0), (1, 0), (0, 4), (1, 5), (0, 8), (1, 10)]
    for (_, _, x), (_, _, y) in zip(fa, fb):
        assert np.array_equal(x, y)
    assert np.array_equal(sa, sb)


@pytest.mark.gpu
def test_gpu_random_scenes_match_the_oracle():
    """tools/fuzz/fuzz_guided.py: random closed and open boundaries of 4 .. 400 segments on either kind, emissive or not, probes
    from half to three scene sizes, trained and guiding samples, three uniform fractions -- fields and counters bit for bit
    (40 seeds were run when the test was written; two stay here: the oracle trains the network on the CPU)"""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz", "fuzz_guided.py"), "3", "2"], capture_output=True, text=True,
                         timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "fuzz guided 3..4: 0 mismatches" in out.stdout, out.stdout[-3000:]
    # the half-precision mode has no bit-exact oracle: on such scenes its fused launch must equal its own per-depth path
    # (fields, counters and the trained weights)
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz", "fuzz_guided.py"), "200", "16", "half"], capture_output=True, text=True,
                         timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "fuzz guided 200..215: 0 mismatches" in out.stdout, out.stdout[-3000:]


# ---- the opt-in training orders (wost_guided_set_option "train_group", "pipeline"): never the parity mode ----------------
REORDERED = [(0, 4), (1, 1), (1, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_reordered_training_keeps_the_guiding_gain(precision):
    """The reordered training orders change WHEN the network learns (a sample sees weights that are a few training passes
    older), not what is estimated: on the bright-disc scene every order must stay unbiased, keep the variance reduction the
    exact order shows (RMSE <= 0.8 x the uniform integrator's at equal samples, not worse than 1.1 x the exact order's),
    take the same number of Adam steps, account for every walk, and be reproducible bit for bit."""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    from elaina_amd.scenes import BRIGHT_DISC_AABB, bright_disc_scene
    p = bright_disc_scene()
    w, depth, eps = 128, 128, 0.05
    it = UniformIntegrator(p, UniformIntegratorSettings((w, w), 8192, depth, eps))
    it.solve()
    ref = it.solution.copy()
    it.close()
    it = UniformIntegrator(p, UniformIntegratorSettings((w, w), 128, depth, eps))
    it.solve()
    rmse_u = float(np.sqrt(np.mean((it.solution - ref) ** 2)))
    it.close()

    def run(pipeline, group):
        st = GuidedIntegratorSettings(frameSize=(w, w), samplesPerPixel=128, trainSppCount=64, maxWalkingDepth=depth, epsilonShell=eps,
                                      batchSize=65536, minBatchSize=8192)
        g = GuidedIntegrator(p, st, BRIGHT_DISC_AABB)
        if precision == 16:
            g.network.set_option("precision", 16)
            g.network.set_option("train_precision", 16)
        g.set_option("pipeline", pipeline)
        g.set_option("train_group", group)
        g.solve()
        out = (g.solution.copy(), g.network.params(), dict(g.last_stats))
        g.close()
        return out

    exact_f, exact_p, exact_s = run(0, 1)
    rmse_exact = float(np.sqrt(np.mean((exact_f - ref) ** 2)))
    assert rmse_exact <= 0.8 * rmse_u
    for pipeline, group in REORDERED:
        f, prm, s = run(pipeline, group)
        f2, prm2, _ = run(pipeline, group)
        assert np.array_equal(f, f2) and np.array_equal(prm, prm2), (pipeline, group)          # reproducible
        assert not np.array_equal(f, exact_f)                                                   # another order of learning
        assert s["optimizer_steps"] == exact_s["optimizer_steps"] > 0
        assert s["walks_started"] == w * w * 128 and s["walks_absorbed"] + s["walks_truncated"] == s["walks_started"]
        rmse = float(np.sqrt(np.mean((f - ref) ** 2)))
        assert rmse <= 0.8 * rmse_u and rmse <= 1.1 * rmse_exact, (pipeline, group, rmse, rmse_exact, rmse_u)
        assert abs(float(f.mean()) - float(ref.mean())) < 0.01 * float(ref.mean())


@pytest.mark.gpu
def test_gpu_reordered_training_is_unbiased_on_the_analytic_problem(oracle):
    """u = y on the unit square (mixed boundary): every training order reproduces it; options are validated"""
    from elaina_amd.capi import WostError
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    w = h = 64
    exact = eval_ys(prob, w, h).reshape(-1)
    errs = {}
    for pipeline, group in [(0, 1)] + REORDERED + [(1, 16)]:
        st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=48, trainSppCount=30, maxWalkingDepth=48, epsilonShell=EPS,
                                      batchSize=4096, minBatchSize=1024)
        gi = GuidedIntegrator(prob, st, AABB, seed=3)
        gi.set_option("pipeline", pipeline)
        gi.set_option("train_group", group)       # 30 trained samples: the last group of 4 / 16 is a short one
        gi.solve()
        e = gi.solution[:, 0] - exact
        assert gi.last_stats["optimizer_steps"] > 0 and gi.last_stats["guided_steps"] > 0
        assert gi.last_stats["walks_started"] == w * h * 48
        assert abs(float(e.mean())) < 4e-3, (pipeline, group, float(e.mean()))
        errs[(pipeline, group)] = float(np.sqrt((e ** 2).mean()))
        gi.close()
    # (with groups of 16 on a second stream none of the 30 trained samples sees a trained network: unbiased all the same, only noisier)
    assert max(v for k, v in errs.items() if k != (1, 16)) < 1.25 * errs[(0, 1)] and errs[(1, 16)] < 2.0 * errs[(0, 1)], errs
    gi = GuidedIntegrator(prob, GuidedIntegratorSettings(frameSize=(8, 8), samplesPerPixel=1, trainSppCount=1, maxWalkingDepth=8,
                                                          epsilonShell=EPS), AABB)
    for key, val in (("pipeline", 2), ("train_group", 0), ("train_group", 17), ("train_group", 1.5), ("no_such_option", 1)):
        with pytest.raises(WostError):
            gi.set_option(key, val)
    gi.close()


@pytest.mark.gpu
def test_gpu_sync_callback_failures_end_the_solve():
    """wost_sync_fn: 0 = done, WOST_SYNC_UNSUPPORTED (2) = op unknown (tolerated for the rank-count op only: a callback
    written against library 0.1), anything else = failure -- of ANY op -- and the solve ends with an error instead of
    training on with a gradient the other ranks do not share"""
    import ctypes as C
    from elaina_amd import capi
    from elaina_amd.capi import WostError
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    st = GuidedIntegratorSettings(frameSize=(32, 32), samplesPerPixel=2, trainSppCount=2, maxWalkingDepth=16, epsilonShell=EPS,
                                  batchSize=1024, minBatchSize=512)

    def solve_with(answers):
        calls = []

        def sync(user, op, data, count):
            calls.append(op)
            rc = answers.get(op, 0)
            if op == capi.SYNC_RANKS_I64_HOST and rc == 0:
                C.cast(data, C.POINTER(C.c_int64))[0] = answers.get("ranks", 1)
            return rc

        gi = GuidedIntegrator(prob, st, AABB, seed=2)
        fn = capi.SYNC_FN(sync)
        capi._check(gi.lib.wost_guided_set_sync(gi._handle, fn, None), "wost_guided_set_sync")
        try:
            gi.solve()
            return gi.last_stats, calls
        finally:
            gi.close()

    s, calls = solve_with({})
    assert s["optimizer_steps"] > 0 and calls[0] == capi.SYNC_RANKS_I64_HOST and capi.SYNC_SUM_I64_DEVICE in calls
    s, _ = solve_with({capi.SYNC_RANKS_I64_HOST: capi.SYNC_UNSUPPORTED})          # a 0.1 callback: undivided gradients, with a warning
    assert s["optimizer_steps"] > 0
    for bad in ({capi.SYNC_RANKS_I64_HOST: 1}, {"ranks": 0}, {capi.SYNC_MIN_I64_HOST: 1}, {capi.SYNC_SUM_I64_DEVICE: 1},
                {capi.SYNC_SUM_I64_DEVICE: capi.SYNC_UNSUPPORTED}):
        with pytest.raises(WostError, match="sync callback failed"):
            solve_with(bad)


@pytest.mark.gpu
def test_gpu_failed_shared_solve_leaves_a_plain_network():
    """The rank count of a shared-network solve belongs to that solve, also when the solve ends in an error: a sync
    callback answers 3 ranks and then fails at the gradient all-reduce, before any optimizer step.  A
    wost_net_train_step on the handle's network afterwards must be the plain step a never-solved handle takes, bit for
    bit (the optimizer divides the gradient by the rank count, and a division by 3 rounds)"""
    import ctypes as C
    from elaina_amd import capi
    from elaina_amd.capi import WostError
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    prob = laplace_box()
    st = GuidedIntegratorSettings(frameSize=(32, 32), samplesPerPixel=2, trainSppCount=2, maxWalkingDepth=16, epsilonShell=EPS,
                                  batchSize=1024, minBatchSize=512)

    def sync(user, op, data, count):
        if op == capi.SYNC_RANKS_I64_HOST:
            C.cast(data, C.POINTER(C.c_int64))[0] = 3
        return 1 if op == capi.SYNC_SUM_I64_DEVICE else 0

    fresh = GuidedIntegrator(prob, st, AABB, seed=2)
    gi = GuidedIntegrator(prob, st, AABB, seed=2)
    fn = capi.SYNC_FN(sync)
    capi._check(gi.lib.wost_guided_set_sync(gi._handle, fn, None), "wost_guided_set_sync")
    try:
        with pytest.raises(WostError, match="gradient all-reduce"):
            gi.solve()
        assert np.array_equal(gi.network.params(), fresh.network.params())      # the solve ended before its first step
        rng = np.random.default_rng(11)
        xy = rng.random((256, 2), dtype=np.float32)
        dl = (0.01 * rng.standard_normal((256, 33))).astype(np.float32)
        p0 = fresh.network.params()
        for it in (gi, fresh):
            it.network.train_step(xy, dl)
        assert not np.array_equal(fresh.network.params(), p0)                   # (the step is a step)
        assert np.array_equal(gi.network.params(), fresh.network.params())
    finally:
        gi.close()
        fresh.close()
