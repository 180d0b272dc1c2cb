"""The fused guided sample kernel past one pixel per lane (guided_sample_kernel, elaina_amd/csrc/wost_guided.hip).

The kernel's grid is sized from the frame (at most 256 blocks of 640 lanes in fp32, 768 in half precision), so on every
frame of test_guided_integrator.py that is compared with a reference a one-sample launch -- every trained sample -- gives no
lane a second pixel, and the wave's 64-item reservation never runs in it.  WOST_GUIDED_MAX_BLOCKS caps that grid: at one block
a 64 x 48 frame gives each lane about five pixels per launch.  What a lane carries from one pixel into the next (begin_walk's
reset), the wave's reservations, the longest-first order and the records of a lane that has walked other pixels are then
compared with the oracle, and the hand-out knobs of DESIGN.md must not change a bit.  "Bit for bit" is the field, the
counters and the network: the trained weights against the oracle, the averaged inference weights and the network
evaluation count (which the oracle does not keep) against the uncapped solve.  Under WOST_GUIDED_DEBUG every fused launch
prints its grid: a capped solve asserts that each of its launches was fused and ran on the capped grid, so that a cap
that no longer applies, or a solve that fell back to the per-depth path, fails instead of passing untested."""
import re

import numpy as np
import pytest

from conftest import wiggly_problem
from oracle.oracle import default_net_config, guided_settings
from test_guided_integrator import AABB, EPS, _band_of_shard_mask, laplace_box
from test_oracle_solver import _poisson_disc

ORACLE_KEYS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps", "train_samples",
               "optimizer_steps")
KEYS = ORACLE_KEYS + ("net_points",)
LADYBUG_AABB = ((-100.0, -100.0), (600.0, 600.0))
KNOBS = ("WOST_GUIDED_MAX_BLOCKS", "WOST_GUIDED_FUSED", "WOST_GUIDED_TAIL_CHUNK", "WOST_GUIDED_TAIL_MARGIN",
         "WOST_GUIDED_SAMPLES_PER_LAUNCH", "WOST_GUIDED_TRAV_BURST", "WOST_GUIDED_WAIT_WEIGHT", "WOST_GUIDED_DEBUG")


def _lobed_params(oracle, seed=3):
    # the random network of test_gpu_frozen_network_matches_oracle (raw outputs in [-2.70, 2.20], kappa <= 6.2: mild lobes)
    rng = np.random.default_rng(seed)
    n = oracle.net_n_params(default_net_config())
    p = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    p[13312:] = rng.uniform(-1, 1, n - 13312).astype(np.float32)
    return p


def _scene(name, ladybug=None):
    """problem and settings of a frame of 3.5 to 6 pixels per lane of one fp32 block"""
    if name == "box":
        return dict(prob=laplace_box(), w=64, h=48, spp=8, train=5, depth=32, eps=EPS, aabb=AABB, batch=2048, min_batch=512, stride=2)
    if name == "ladybug":
        # ragged: the first launch hands the pixels out row by row
        return dict(prob=ladybug, w=75, h=53, spp=5, train=3, depth=48, eps=1.0, aabb=LADYBUG_AABB, batch=2048, min_batch=512)
    if name == "wiggly":
        # 3000-segment emissive Neumann boundary on the tree
        return dict(prob=wiggly_problem(emissive=True), w=52, h=44, spp=4, train=2, depth=32, eps=EPS, aabb=((-140.0, -140.0), (140.0, 140.0)),
                    batch=1024, min_batch=256)
    if name == "source":
        return dict(prob=_poisson_disc(), w=56, h=56, spp=5, train=3, depth=48, eps=EPS, aabb=((-1.2, -1.2), (1.2, 1.2)), batch=2048,
                    min_batch=512)
    if name == "masked":
        # ragged, every fifth pixel masked out, training pixel stride with an offset
        prob = laplace_box()
        prob.mask = (np.arange(67 * 45) % 5 != 0).astype(np.uint8)
        return dict(prob=prob, w=67, h=45, spp=6, train=4, depth=32, eps=EPS, aabb=AABB, batch=512, min_batch=128, stride=2, offset=1)
    raise ValueError(name)


def _settings(sc):
    from elaina_amd.guided import GuidedIntegratorSettings
    return GuidedIntegratorSettings(frameSize=(sc["w"], sc["h"]), samplesPerPixel=sc["spp"], trainSppCount=sc["train"],
                                    maxWalkingDepth=sc["depth"], epsilonShell=sc["eps"], batchSize=sc["batch"], minBatchSize=sc["min_batch"],
                                    trainPixelStride=sc.get("stride", 1), trainPixelOffset=sc.get("offset", 0),
                                    uniformFractionInTrainingPhase=sc.get("uf", (0.5, 0.5))[0],
                                    uniformFractionInGuidingPhase=sc.get("uf", (0.5, 0.5))[1])


def _fused_blocks(capfd):
    """the grid of every fused launch since the last call, from the WOST_GUIDED_DEBUG lines on stderr"""
    return [int(b) for b in re.findall(r"^\[fused sample \d+ x\d+\] (\d+) blocks", capfd.readouterr().err, re.M)]


def _gpu(monkeypatch, sc, env=None, precision=32, walk_order=None, params=None, solves=1, shard=None, seed=7, capfd=None, blocks=None):
    """solve(s) of one handle under the knobs `env` (every other knob unset): [(field, stats, params, inference params)] and the
    weights the handle started from.  With `capfd`, every launch of every solve must have been a fused launch of `blocks` blocks."""
    import torch
    from elaina_amd.guided import GuidedIntegrator
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    if capfd is not None:
        monkeypatch.setenv("WOST_GUIDED_DEBUG", "1")
        capfd.readouterr()
    gi = GuidedIntegrator(sc["prob"], _settings(sc), sc["aabb"], seed=seed)
    if params is not None:
        gi.network.set_params(params)
    p0 = gi.network.params()
    if precision == 16:
        gi.network.set_option("precision", 16)
        gi.network.set_option("train_precision", 16)
    if walk_order is not None:
        gi.set_option("walk_order", walk_order)
    out = []
    for _ in range(solves):
        if shard is None:
            gi.solve()
            f = gi.solution.copy()
        else:
            buf = torch.full((sc["w"] * sc["h"] * 3,), 7.0, device="cuda")     # must be overwritten, other shards' pixels with 0
            gi.solve_sharded(shard[0], shard[1], buf.data_ptr())
            torch.cuda.synchronize()
            f = buf.cpu().numpy().reshape(-1, 3)
        out.append((f, {k: gi.last_stats[k] for k in KEYS}, gi.network.params(), gi.network.inference_params()))
        if capfd is not None:
            grids = _fused_blocks(capfd)
            assert grids and set(grids) == {blocks}, (blocks, grids)
    gi.close()
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return out, p0


def _oracle(oracle, sc, params):
    """the oracle's field and counters, and the network it trained from `params`"""
    gs = guided_settings(sc["w"], sc["h"], sc["spp"], sc["depth"], sc["eps"], sc["aabb"][0], sc["aabb"][1], train_spp_count=sc["train"],
                         batch_size=sc["batch"], min_batch_size=sc["min_batch"], train_pixel_stride=sc.get("stride", 1),
                         train_pixel_offset=sc.get("offset", 0), uniform_fraction=sc.get("uf", (0.5, 0.5)))
    sd = sc["prob"].as_dict()
    if sc.get("mask") is not None:
        sd["mask"] = sc["mask"]
    p = params.copy()
    ref = oracle.solve_guided(sd, gs, default_net_config(), p, threads=16)
    return ref, p


def _same(a, b, what, keys=KEYS):
    """two GPU solves (field, stats, params, inference params) agree bit for bit"""
    (fa, sa, pa, ia), (fb, sb, pb, ib) = a, b
    for k in keys:
        assert sa[k] == sb[k], (what, k, sa[k], sb[k])
    assert np.array_equal(pa, pb) and np.array_equal(ia, ib), what
    assert np.array_equal(fa, fb), (what, float(np.abs(fa - fb).max()))


def _matches_oracle(got, ref, p_ref, what):
    f, s, p, _ = got
    for k in ORACLE_KEYS:
        assert s[k] == ref[k], (what, k, s[k], ref[k])
    assert np.array_equal(f, ref["field"]), (what, float(np.abs(f - ref["field"]).max()))
    assert np.array_equal(p, p_ref), what


# ---- a. capped fp32 solves against the oracle -------------------------------------------------------------------------
# per scene the capped solves that share one oracle solve: the grid (blocks) and the handle's walk_order (0: the frame's own
# order, tiled or row by row, in every launch; default 1: longest walks first from the second one-sample launch on)
CAPPED = {
    "box": [dict(cap=1), dict(cap=2)],
    "ladybug": [dict(cap=1)],
    "wiggly": [dict(cap=1)],
    "source": [dict(cap=1)],
    "masked": [dict(cap=1, walk_order=0), dict(cap=2)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(CAPPED))
def test_gpu_capped_guided_solve_matches_oracle(oracle, ladybug, monkeypatch, capfd, scene):
    """trained samples (one launch each) and then the guiding samples in one launch, on a grid of one or two blocks: every
    lane walks pixel after pixel, and the field, the counters and the trained network are the oracle's"""
    sc = _scene(scene, ladybug)
    ref = p_ref = None
    for run in CAPPED[scene]:
        assert sc["w"] * sc["h"] >= 2 * 640 * run["cap"]            # at least two pixels per lane in a one-sample launch
        (capped,), p0 = _gpu(monkeypatch, sc, {"WOST_GUIDED_MAX_BLOCKS": run["cap"]}, walk_order=run.get("walk_order"), capfd=capfd,
                             blocks=run["cap"])
        assert capped[1]["optimizer_steps"] > 0 and capped[1]["guided_steps"] > 0
        if ref is None:
            ref, p_ref = _oracle(oracle, sc, p0)
        _matches_oracle(capped, ref, p_ref, run)
        _same(capped, _gpu(monkeypatch, sc, walk_order=run.get("walk_order"))[0][0], run)
        if sc["prob"].mask is not None:
            assert not capped[0][sc["prob"].mask == 0].any()
    if scene == "wiggly":
        assert ref["neumann_hits"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["box", "wiggly"])
def test_gpu_capped_first_pass_records_match_oracle(oracle, monkeypatch, capfd, scene):
    """one trained sample and no Adam step on one block: the ordered training set -- every record of a lane that has walked
    other pixels before, the normal and the Neumann flag of a walk's first vertex included -- is the oracle's"""
    from elaina_amd.guided import GuidedIntegrator
    sc = dict(_scene(scene), spp=1, train=1, min_batch=10 ** 9)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WOST_GUIDED_MAX_BLOCKS", "1")
    monkeypatch.setenv("WOST_GUIDED_DEBUG", "1")
    capfd.readouterr()
    gi = GuidedIntegrator(sc["prob"], _settings(sc), sc["aabb"], seed=7)
    p0 = gi.network.params()
    gi.solve()
    ts, f, s = gi.train_set(), gi.solution.copy(), dict(gi.last_stats)
    gi.close()
    assert _fused_blocks(capfd) == [1]
    gs = guided_settings(sc["w"], sc["h"], 1, sc["depth"], sc["eps"], sc["aabb"][0], sc["aabb"][1], train_spp_count=1, batch_size=sc["batch"],
                         min_batch_size=sc["min_batch"], train_pixel_stride=sc.get("stride", 1))
    ref = oracle.solve_guided(sc["prob"].as_dict(), gs, default_net_config(), p0.copy(), threads=16, dump_spp=0)
    to = ref["train_set"]
    assert s["optimizer_steps"] == 0 and s["train_samples"] == len(ts["xy"]) == len(to["xy"]) == ref["train_samples"] > 0
    assert np.array_equal(f, ref["field"])
    for k in ("xy", "dir", "solution", "dir_pdf", "normal", "on_neumann"):
        assert np.array_equal(ts[k], to[k]), k
    for k in ORACLE_KEYS:
        assert s[k] == ref[k], k
    if scene == "wiggly":
        assert to["on_neumann"].any()


@pytest.mark.gpu
def test_gpu_capped_frozen_one_sample_launches_match_oracle(oracle, monkeypatch, capfd):
    """no training, WOST_GUIDED_SAMPLES_PER_LAUNCH=1: every guiding sample is a launch of its own, from the second one on in
    the longest-first order, and a lane walks about five pixels in each"""
    sc = dict(_scene("box"), spp=4, train=0)
    p = _lobed_params(oracle)
    got = _gpu(monkeypatch, sc, {"WOST_GUIDED_MAX_BLOCKS": 1, "WOST_GUIDED_SAMPLES_PER_LAUNCH": 1}, params=p, capfd=capfd, blocks=1)[0][0]
    ref, p_ref = _oracle(oracle, sc, p)
    assert ref["guided_steps"] > 0 and ref["optimizer_steps"] == 0
    _matches_oracle(got, ref, p_ref, "frozen")
    assert np.array_equal(got[2], p)
    _same(got, _gpu(monkeypatch, sc, {"WOST_GUIDED_SAMPLES_PER_LAUNCH": 1}, params=p)[0][0], "frozen")


# ---- b. the hand-out knobs -------------------------------------------------------------------------------------------
# at one block of 640 lanes the tail margin is pct * 6 items: 300 % = 1800 of a one-sample launch's 3072 (the first
# reservations 64 at a time, then the tail), 0 = never the tail, 100000 = the tail from the first reservation; chunk 0 = no tail
HANDOUT = [
    dict(TAIL_CHUNK=0, SAMPLES_PER_LAUNCH=1, walk_order=0),
    dict(TAIL_CHUNK=1, TAIL_MARGIN=100000, TRAV_BURST=1),
    dict(TAIL_CHUNK=4, TAIL_MARGIN=0, SAMPLES_PER_LAUNCH=3, WAIT_WEIGHT=512),
    dict(TAIL_CHUNK=64, TAIL_MARGIN=100000, SAMPLES_PER_LAUNCH=1, TRAV_BURST=16),
    dict(TAIL_CHUNK=4, TAIL_MARGIN=300, SAMPLES_PER_LAUNCH=64, TRAV_BURST=16, WAIT_WEIGHT=1),
    dict(TAIL_CHUNK=1, TAIL_MARGIN=300, SAMPLES_PER_LAUNCH=3, TRAV_BURST=1, WAIT_WEIGHT=1, walk_order=0),
    dict(TAIL_CHUNK=0, TAIL_MARGIN=100000, SAMPLES_PER_LAUNCH=64, WAIT_WEIGHT=512),
    dict(TAIL_CHUNK=64, TAIL_MARGIN=0, SAMPLES_PER_LAUNCH=1, TRAV_BURST=1, WAIT_WEIGHT=512),
]


@pytest.mark.gpu
def test_gpu_guided_handout_knobs_change_no_bit(oracle, monkeypatch, capfd):
    """the tail reservations, the samples per guiding launch and the scheduler's weights decide which lane walks which
    pixel when, never what a walk computes: eight combinations on one block, two of them in the frame's tiled order, all
    equal the oracle"""
    sc = dict(_scene("box"), spp=8, train=3)
    ref = p_ref = first = None
    for knobs in HANDOUT:
        env = {"WOST_GUIDED_" + k: v for k, v in knobs.items() if k != "walk_order"}
        env["WOST_GUIDED_MAX_BLOCKS"] = 1
        (got,), p0 = _gpu(monkeypatch, sc, env, walk_order=knobs.get("walk_order"), capfd=capfd, blocks=1)
        if ref is None:
            ref, p_ref = _oracle(oracle, sc, p0)
        _matches_oracle(got, ref, p_ref, knobs)
        if first is None:
            first = got
        _same(got, first, knobs)


# ---- c. half precision: capped fused launches against the per-depth path ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["box", "wiggly"])
def test_gpu_capped_half_precision_equals_the_per_depth_launches(monkeypatch, capfd, scene):
    """the half-precision mode has no bit-exact oracle: one block of 768 lanes (about four pixels each in a one-sample launch)
    against WOST_GUIDED_FUSED=0"""
    sc = _scene(scene)
    capped = _gpu(monkeypatch, sc, {"WOST_GUIDED_MAX_BLOCKS": 1}, precision=16, capfd=capfd, blocks=1)[0][0]
    per_depth = _gpu(monkeypatch, sc, {"WOST_GUIDED_FUSED": 0}, precision=16)[0][0]
    assert capped[1]["optimizer_steps"] > 0 and capped[1]["guided_steps"] > 0 and np.isfinite(capped[0]).all()
    _same(capped, per_depth, scene)


@pytest.mark.gpu
def test_gpu_capped_half_precision_solve_repeated_on_one_handle(monkeypatch, capfd):
    """the second solve of a handle starts from the first one's network and its cached evaluation-point queries"""
    sc = dict(_scene("box"), spp=5, train=3)
    capped = _gpu(monkeypatch, sc, {"WOST_GUIDED_MAX_BLOCKS": 1}, precision=16, solves=2, capfd=capfd, blocks=1)[0]
    per_depth = _gpu(monkeypatch, sc, {"WOST_GUIDED_FUSED": 0}, precision=16, solves=2)[0]
    for k in range(2):
        _same(capped[k], per_depth[k], "solve %d" % k)
    assert not np.array_equal(capped[0][2], capped[1][2])


# ---- d. shards with a cap ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_capped_frozen_shards_sum_to_the_oracle(oracle, monkeypatch, capfd):
    """three capped shards of a frozen solve, one launch per sample: a lane asks for about five pixels of which one in three
    is its shard's; the shards sum to the oracle's full frame"""
    sc = dict(_scene("box"), spp=4, train=0)
    p = _lobed_params(oracle, 5)
    env = {"WOST_GUIDED_MAX_BLOCKS": 1, "WOST_GUIDED_SAMPLES_PER_LAUNCH": 1}
    total = np.zeros((sc["w"] * sc["h"], 3), np.float32)
    sums = dict.fromkeys(ORACLE_KEYS, 0)
    for r in range(3):
        f, s, _, _ = _gpu(monkeypatch, sc, env, params=p, shard=(r, 3), capfd=capfd, blocks=1)[0][0]
        total += f
        for k in ORACLE_KEYS:
            sums[k] += s[k]
    ref, _ = _oracle(oracle, sc, p)
    assert np.array_equal(total, ref["field"]), float(np.abs(total - ref["field"]).max())
    for k in ORACLE_KEYS:
        assert sums[k] == ref[k], (k, sums[k], ref[k])


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_capped_trained_shard_equals_uncapped_and_per_depth(monkeypatch, capfd, precision):
    """shard 1 of 3 with training: capped, uncapped and per-depth solves of the shard agree bit for bit"""
    sc = dict(_scene("box"), spp=6, train=3)
    capped = _gpu(monkeypatch, sc, {"WOST_GUIDED_MAX_BLOCKS": 1}, precision=precision, shard=(1, 3), capfd=capfd, blocks=1)[0][0]
    assert capped[1]["optimizer_steps"] > 0
    _same(capped, _gpu(monkeypatch, sc, precision=precision, shard=(1, 3))[0][0], "uncapped")
    _same(capped, _gpu(monkeypatch, sc, {"WOST_GUIDED_FUSED": 0}, precision=precision, shard=(1, 3))[0][0], "per depth")


# ---- e. config 4's frame on the default grid ------------------------------------------------------------------------------
def _config4(ladybug, spp, train):
    return dict(prob=ladybug, w=1024, h=1024, spp=spp, train=train, depth=64, eps=1.0, aabb=LADYBUG_AABB, batch=524288, min_batch=65536)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [32, 16])
def test_gpu_config4_frame_fused_equals_per_depth(ladybug, monkeypatch, capfd, precision):
    """ladybug at 1024^2 with the reference's batch sizes, 2 trained + 2 guiding samples, on the default grid of 256 blocks:
    each lane walks five to six pixels per one-sample launch, in the longest-first order from the second launch on"""
    sc = _config4(ladybug, 4, 2)
    fused = _gpu(monkeypatch, sc, precision=precision, seed=42, capfd=capfd, blocks=256)[0][0]
    per_depth = _gpu(monkeypatch, sc, {"WOST_GUIDED_FUSED": 0}, precision=precision, seed=42)[0][0]
    assert fused[1]["optimizer_steps"] == 2 * 5 and fused[1]["walks_started"] == 4 * 1024 * 1024
    _same(fused, per_depth, precision)


@pytest.mark.gpu
def test_gpu_config4_frame_one_sample_launches_band_matches_oracle(oracle, ladybug, monkeypatch, capfd):
    """a frozen 1024^2 solve with one launch per sample (the longest-first order from the second on): the 8-row band of the
    largest mean Dirichlet distance -- the longest walks, the last pixels of the order -- and the middle band against the
    oracle, which walks only those two bands (a mask; with a frozen network a pixel depends on no other pixel)"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    sc = _config4(ladybug, 4, 0)
    f, s, p, _ = _gpu(monkeypatch, sc, {"WOST_GUIDED_SAMPLES_PER_LAUNCH": 1}, seed=42, capfd=capfd, blocks=256)[0][0]
    assert s["walks_started"] == 4 * 1024 * 1024 and s["guided_steps"] > 0 and s["optimizer_steps"] == 0
    ui = UniformIntegrator(ladybug, UniformIntegratorSettings((1024, 1024), 1, 64, 1.0))
    band = int(np.argmax(ui.renderDirichletSDF().reshape(128, 8 * 1024).mean(axis=1)))
    ui.close()
    mask, _, _ = _band_of_shard_mask(1024, 1024, 8, 0, 1)
    mask[band * 8 * 1024:(band + 1) * 8 * 1024] = 1
    ref, _ = _oracle(oracle, dict(sc, mask=mask), p)
    sel = mask.astype(bool)
    assert ref["walks_started"] == int(sel.sum()) * 4 and int(sel.sum()) == 2 * 8 * 1024
    assert np.array_equal(f[sel], ref["field"][sel]), (band, float(np.abs(f[sel] - ref["field"][sel]).max()))
