"""Guided solves at the caller's evaluation points (wost_guided_solve_points & co.), bit for bit (np.array_equal throughout).

Three references:
  the frame solve of the same build (itself pinned to the oracle by test_guided_integrator.py / test_guided_3d.py): the frame's
      own evaluation points must reproduce it -- field, counters, training sets, trained weights;
  the oracle's frame solve with ANOTHER probe, whose evaluation grid is the point list: trained point solves at points that are
      not the handle's grid, with n < width * height and seed_width != width;
  the oracle's solve with a zero-scale probe at p and a frozen network: entry k of its field is point p on the random stream of
      pixel k (the oracle's guided solve has no per-pixel counters: these compare the field).
The oracle's own figures are asserted first, so that a changed fixture is noticed."""
import numpy as np
import pytest

from conftest import box_problem, cube_scene3
from oracle.oracle import default_net_config, default_net_config3, guided_settings, guided_settings3
from test_gpu_points import _grid_points, _mixed_box
from test_guided_3d import AABB3, _hip_cfg, _rand_params3
from test_guided_integrator import AABB, EPS, init_params, laplace_box

pytestmark = pytest.mark.gpu

COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps", "train_samples", "optimizer_steps")
WALK_COUNTERS = COUNTERS[:6]
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _gi2(prob, w, h, spp, train_spp, depth=32, batch=2048, min_batch=512, stride=1, offset=0, params=None, seed=7, precision=None):
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=train_spp, maxWalkingDepth=depth, epsilonShell=EPS,
                                  batchSize=batch, minBatchSize=min_batch, trainPixelStride=stride, trainPixelOffset=offset)
    gi = GuidedIntegrator(prob, st, AABB, seed=seed)
    if precision is not None:
        gi.network.set_option("precision", precision)
    if params is not None:
        gi.network.set_params(params)
    return gi


def _same_train_sets(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 2-D ---------------------------------------------------------------------------------------------------------------------
# 1. the frame's own points, trained
@pytest.mark.parametrize("w,h,fused", [(40, 33, None), (48, 40, None), (40, 33, "0"), (48, 40, "0")],
                         ids=["40x33", "48x40-tiles", "40x33-per-depth", "48x40-tiles-per-depth"])
def test_the_frames_own_points_reproduce_the_trained_frame_solve(oracle, monkeypatch, w, h, fused):
    """40 x 33 is not made of whole 8 x 8 tiles; at 48 x 40 the frame path permutes its queue by tiles and the point path
    keeps the order of the list.  WOST_GUIDED_FUSED=0: the launches per depth"""
    if fused is not None:
        monkeypatch.setenv("WOST_GUIDED_FUSED", fused)
    prob = laplace_box()
    grid = _once(("grid", w, h), lambda: _grid_points(oracle, prob, w, h))
    a, b = _gi2(prob, w, h, 6, 4), _gi2(prob, w, h, 6, 4)
    a.solve()
    field = b.solve_points(grid)
    for k in COUNTERS:
        assert a.last_stats[k] == b.last_stats[k], k
    assert a.last_stats["optimizer_steps"] > 0 and a.last_stats["train_samples"] > 0 and a.last_stats["walks_started"] == 6 * w * h
    assert np.any(field != 0) and np.array_equal(field, a.solution)
    _same_train_sets(a.train_set(), b.train_set())
    assert np.array_equal(a.network.params(), b.network.params())
    a.close()
    b.close()


# 2. another probe's grid, trained, against the oracle
OTHER_PROBE = (0.3, 0.52, 0.47, 0.6, 0.8)
OTHER_FIGURES = {
    (1, 0): dict(walk_steps=31496, walks_started=2880, walks_absorbed=2840, walks_truncated=40, neumann_hits=1661, guided_steps=10521,
                 train_samples=5580, optimizer_steps=12, last_set=1406),
    (3, 2): dict(walk_steps=32368, train_samples=1853, optimizer_steps=4, last_set=464),
}


def _other_probe_problem():
    return box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.0, n_per_side=8, probe=OTHER_PROBE)


def _other_probe_ref(oracle, stride, offset):
    def make():
        cfg = default_net_config()
        prob = _other_probe_problem()
        gs = guided_settings(24, 20, 6, 32, EPS, AABB[0], AABB[1], train_spp_count=4, batch_size=512, min_batch_size=128,
                             train_pixel_stride=stride, train_pixel_offset=offset)
        trained = init_params(oracle, cfg, 7)
        ref = oracle.solve_guided(prob.as_dict(), gs, cfg, trained, threads=16, dump_spp=3)
        ref["params"] = trained
        want = OTHER_FIGURES[(stride, offset)]
        for k, v in want.items():
            got = len(ref["train_set"]["xy"]) if k == "last_set" else ref[k]
            assert got == v, (k, got, v)
        return ref
    return _once(("other", stride, offset), make)


@pytest.mark.parametrize("stride,offset", [(1, 0), (3, 2)])
def test_another_probes_grid_trained_matches_the_oracle(oracle, stride, offset):
    """480 points on a 32 x 32 handle, seeds of a frame 24 wide: the list trains one network exactly as the oracle's 24 x 20
    frame does; training points by the index in the call (stride 3 from offset 2)"""
    ref = _other_probe_ref(oracle, stride, offset)
    pts = _once("other-grid", lambda: _grid_points(oracle, _other_probe_problem(), 24, 20))
    assert not np.array_equal(pts, _grid_points(oracle, laplace_box(), 24, 20))
    gi = _gi2(laplace_box(), 32, 32, 6, 4, batch=512, min_batch=128, stride=stride, offset=offset, params=init_params(oracle, default_net_config(), 7))
    field = gi.solve_points(pts, 0, 24)
    for k in COUNTERS:
        assert gi.last_stats[k] == ref[k], (k, gi.last_stats[k], ref[k])
    assert np.array_equal(field, ref["field"]), float(np.abs(field - ref["field"]).max())
    _same_train_sets(gi.train_set(), ref["train_set"])
    assert np.array_equal(gi.network.params(), ref["params"])
    gi.close()


# 3. arbitrary points, frozen network
def _points2(n=70):
    pts = np.random.default_rng(11).uniform(0.02, 0.98, (n, 2)).astype(np.float32)
    pts[0] = pts[1] = (0.5, 0.0)      # a mesh vertex, twice: equal coordinates, different streams
    pts[2] = (1.0, 0.5)               # on the Neumann side
    pts[3] = (0.5, 0.5)
    pts[4] = (1.5, 0.5)               # outside the domain and the guiding box
    pts[5] = (0.5, -0.25)
    return pts


def _frozen_params2(oracle):
    """the frozen weights of test_gpu_frozen_network_matches_oracle"""
    rng = np.random.default_rng(3)
    n = oracle.net_n_params(default_net_config())
    p = rng.uniform(-0.3, 0.3, n).astype(np.float32)
    p[13312:] = rng.uniform(-1, 1, n - 13312).astype(np.float32)
    return p


FROZEN2 = dict(seed_base=5, seed_width=16, spp=4, depth=32)


def _frozen_ref2(oracle, n=70):
    """one oracle solve per point: a 16 x 5 frame whose zero-scale probe sits at the point, no training; entry seed_base + i"""
    def make():
        cfg, params, sd = default_net_config(), _frozen_params2(oracle), _mixed_box().as_dict()
        gs = guided_settings(16, 5, FROZEN2["spp"], FROZEN2["depth"], EPS, AABB[0], AABB[1], train_spp_count=0)
        out = np.zeros((n, 3), np.float32)
        for i, p in enumerate(_points2(n)):
            sd["probe"] = (0.0, float(p[0]), float(p[1]), 0.0, 1.0)
            w = params.copy()
            out[i] = oracle.solve_guided(sd, gs, cfg, w, threads=4)["field"][FROZEN2["seed_base"] + i]
            assert np.array_equal(w, params)
        return out
    return _once(("frozen2", n), make)


@pytest.fixture(scope="module")
def frozen2(oracle):
    ref = _frozen_ref2(oracle)
    assert np.all(np.isfinite(ref)) and np.all(np.any(ref != 0, axis=1))
    assert ref[0, 0] != ref[1, 0]
    assert abs(float(ref[:, 0].astype(np.float64).sum()) - 148.84869) < 1e-4, float(ref[:, 0].astype(np.float64).sum())
    return ref


def _frozen_gi2(oracle, train_spp=4, spp=FROZEN2["spp"]):
    return _gi2(_mixed_box(), 16, 16, spp, train_spp, depth=FROZEN2["depth"], params=_frozen_params2(oracle))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70])
def test_arbitrary_points_with_a_frozen_network_match_the_oracle(oracle, frozen2, n):
    """the handle trains four samples; train_spp = 0 overrides that for the call: guiding-phase settings from the first sample
    on, the weights untouched.  n around the cursor reservations of 64"""
    gi = _frozen_gi2(oracle)
    p0 = gi.network.params()
    field = gi.solve_points(_points2()[:n], FROZEN2["seed_base"], FROZEN2["seed_width"], train_spp=0)
    assert field.dtype == np.float32 and np.array_equal(field, frozen2[:n]), float(np.abs(field - frozen2[:n]).max())
    assert gi.last_stats["optimizer_steps"] == 0 == gi.last_stats["train_samples"]
    assert gi.last_stats["walks_started"] == n * FROZEN2["spp"] and gi.last_stats["guided_steps"] > 0
    assert np.array_equal(gi.network.params(), p0)
    gi.close()


def test_a_cut_list_gives_the_same_rows(oracle, frozen2):
    gi = _frozen_gi2(oracle)
    pts = _points2()
    a = gi.solve_points(pts[:33], FROZEN2["seed_base"], FROZEN2["seed_width"], train_spp=0)
    b = gi.solve_points(pts[33:], FROZEN2["seed_base"] + 33, FROZEN2["seed_width"], train_spp=0)
    assert np.array_equal(np.concatenate([a, b]), frozen2)
    gi.close()


# 4. half precision, frozen
def test_half_precision_frozen_points_reproduce_the_frame_solve(oracle):
    """the fused half-precision kernel with handed samples (five samples of every pixel in one launch)"""
    prob = laplace_box()
    grid = _once(("grid", 48, 40), lambda: _grid_points(oracle, prob, 48, 40))
    gi = _gi2(prob, 48, 40, 5, 0, precision=16)
    gi.solve()
    want, stats = gi.solution.copy(), dict(gi.last_stats)
    field = gi.solve_points(grid, train_spp=0)
    for k in COUNTERS:
        assert gi.last_stats[k] == stats[k], k
    assert stats["guided_steps"] > 0 and np.any(want != 0) and np.array_equal(field, want)
    gi.close()


# 5. no leakage
def test_a_point_solve_between_two_frame_solves_leaves_the_second_what_it_was(oracle):
    """the cached depth-0 queries, the hints, the order buffers and the pixel state words belong to one solve"""
    gi = _frozen_gi2(oracle, train_spp=0)
    gi.solve()
    want, stats = gi.solution.copy(), dict(gi.last_stats)
    gi.solve_points(_points2(100), FROZEN2["seed_base"], FROZEN2["seed_width"])
    assert gi.last_stats["walks_started"] == 100 * FROZEN2["spp"]
    gi.solve()
    for k in COUNTERS:
        assert gi.last_stats[k] == stats[k], k
    assert np.any(want != 0) and np.array_equal(gi.solution, want)
    gi.close()


# 6. device arrays and refusals
def test_device_arrays_and_refusals(oracle, frozen2):
    import torch
    from elaina_amd import capi
    gi = _frozen_gi2(oracle)
    kw = dict(seed_base=FROZEN2["seed_base"], seed_width=FROZEN2["seed_width"], train_spp=0)
    host = gi.solve_points(_points2(), **kw)
    host_stats = dict(gi.last_stats)
    assert np.array_equal(host, frozen2)
    pts = torch.from_numpy(_points2()).cuda()
    field = torch.full((len(pts), 3), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stats = gi.solve_points_dev(pts.data_ptr(), len(pts), field.data_ptr(), **kw)
    assert np.array_equal(field.cpu().numpy(), host)
    for k in COUNTERS:
        assert stats[k] == host_stats[k], k
    # a point that is not finite is never walked: a NaN row, the other rows unchanged
    bad = _points2()
    bad[37, 1] = np.nan
    pts = torch.from_numpy(bad).cuda()
    field.fill_(-1.0)
    torch.cuda.synchronize()
    stats = gi.solve_points_dev(pts.data_ptr(), len(pts), field.data_ptr(), **kw)
    got = field.cpu().numpy()
    assert np.all(np.isnan(got[37])) and np.array_equal(np.delete(got, 37, 0), np.delete(host, 37, 0))
    assert stats["walks_started"] == host_stats["walks_started"] - FROZEN2["spp"]
    # refusals: the capacity of the handle, a host point that is not finite
    with pytest.raises(capi.WostError, match="256"):
        gi.solve_points(np.full((257, 2), 0.5, np.float32), **kw)
    assert gi.solve_points(np.full((256, 2), 0.5, np.float32), **kw).shape == (256, 3)
    with pytest.raises(capi.WostError, match="point 37 "):
        gi.solve_points(bad, **kw)
    with pytest.raises(capi.WostError, match="train_spp_count"):
        gi.solve_points(_points2(), train_spp=-2)
    assert gi.solve_points(np.zeros((0, 2), np.float32)).shape == (0, 3)
    gi.close()


# ---- 3-D ---------------------------------------------------------------------------------------------------------------------
def _cfg3():
    return default_net_config3(n_levels=4)


def _scene3(probe=None):
    return cube_scene3(n=3, d_faces=(4, 5), n_faces=(0, 1, 2, 3), value=lambda x, y, z: z, flux=lambda x, y, z, f: 0.3 * (f - 1.5), probe=probe)


def _gi3(orc, sd, w, h, spp, train_spp, depth=48, batch=256, min_batch=64, stride=1, offset=0):
    from elaina_amd.guided import GuidedIntegratorSettings
    from elaina_amd.integrator3d import GuidedIntegrator3, Problem3
    st = GuidedIntegratorSettings(frameSize=(w, h), samplesPerPixel=spp, trainSppCount=train_spp, maxWalkingDepth=depth, epsilonShell=EPS,
                                  batchSize=batch, minBatchSize=min_batch, trainPixelStride=stride, trainPixelOffset=offset)
    gi = GuidedIntegrator3(Problem3.from_dict(sd), st, AABB3, network_config=_hip_cfg(_cfg3()), seed=7)
    gi.network.set_params(_rand_params3(orc, _cfg3(), seed=5))
    return gi


def _grid3(w, h, at):
    """the evaluation grid of a probe of scale 0.25 whose right / up are coordinate axes: 0.25 * ndc + pos, exact in float32"""
    py, px = np.divmod(np.arange(w * h), w)
    ndcx, ndcy = (2.0 * px / w - 1.0).astype(np.float32), (2.0 * py / h - 1.0).astype(np.float32)
    return at(np.float32(0.25) * ndcx, np.float32(0.25) * ndcy).astype(np.float32)


# 7. the frame's own points
@pytest.mark.parametrize("fused", ["1", "0"])
def test_3d_the_frames_own_points_reproduce_the_trained_frame_solve(oracle, monkeypatch, fused):
    monkeypatch.setenv("WOST3_G_FUSED", fused)
    sd = _scene3(probe=(0.25, (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
    pts = _grid3(32, 32, lambda u, v: np.stack([np.float32(0.5) + u, np.float32(0.5) + v, np.full(len(u), 0.5, np.float32)], 1))
    a, b = _gi3(oracle, sd, 32, 32, 6, 4), _gi3(oracle, sd, 32, 32, 6, 4)
    a.solve()
    field = b.solve_points(pts, 0, 32)
    for k in COUNTERS:
        assert a.last_stats[k] == b.last_stats[k], k
    assert a.last_stats["optimizer_steps"] > 0 and a.last_stats["walks_started"] == 6 * 32 * 32
    assert np.any(field != 0) and np.array_equal(field, a.solution)
    _same_train_sets(a.train_set(), b.train_set())
    assert np.array_equal(a.network.params(), b.network.params())
    a.close()
    b.close()


# 8. another probe's grid, trained, against the oracle
OTHER3_FIGURES = dict(walk_steps=31973, walks_started=1536, walks_absorbed=1472, walks_truncated=64, neumann_hits=2343, guided_steps=7127,
                      train_samples=1018, optimizer_steps=4, last_set=255)


def test_3d_another_probes_grid_trained_matches_the_oracle(oracle):
    """256 points of the slice x = 0.375 on a 20 x 16 handle whose own probe is the slice z = 0.5; training points every third
    from offset 1"""
    sd = _scene3(probe=(0.25, (0.375, 0.5, 0.5), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)))
    gs = guided_settings3(16, 16, 6, 48, EPS, AABB3[0], AABB3[1], train_spp_count=4, batch_size=256, min_batch_size=64,
                          train_pixel_stride=3, train_pixel_offset=1)
    trained = _rand_params3(oracle, _cfg3(), seed=5)
    ref = oracle.solve_guided3(sd, gs, _cfg3(), trained, threads=16, dump_spp=3)
    for k, v in OTHER3_FIGURES.items():
        got = len(ref["train_set"]["xyz"]) if k == "last_set" else ref[k]
        assert got == v, (k, got, v)
    assert abs(float(ref["field"].astype(np.float64).mean()) - 0.5015) < 5e-5, float(ref["field"].astype(np.float64).mean())
    pts = _grid3(16, 16, lambda u, v: np.stack([np.full(len(u), 0.375, np.float32), np.float32(0.5) + u, np.float32(0.5) + v], 1))
    gi = _gi3(oracle, _scene3(), 20, 16, 6, 4, stride=3, offset=1)
    field = gi.solve_points(pts, 0, 16)
    for k in COUNTERS:
        assert gi.last_stats[k] == ref[k], (k, gi.last_stats[k], ref[k])
    assert np.array_equal(field, ref["field"]), float(np.abs(field - ref["field"]).max())
    _same_train_sets(gi.train_set(), ref["train_set"])
    assert np.array_equal(gi.network.params(), trained)
    gi.close()


# 9. volumetric points, frozen
def _points3():
    return np.random.default_rng(3).uniform(-0.1, 1.1, (40, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def frozen3(oracle):
    pts = _points3()
    assert int(np.all((pts > 0) & (pts < 1), axis=1).sum()) == 27
    cfg, params, sd = _cfg3(), _rand_params3(oracle, _cfg3(), seed=5), _scene3()
    gs = guided_settings3(16, 3, 3, 48, EPS, AABB3[0], AABB3[1], train_spp_count=0)
    ref = np.zeros((len(pts), 3), np.float32)
    for i, p in enumerate(pts):
        sd["probe"] = (0.0, tuple(float(v) for v in p), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))
        ref[i] = oracle.solve_guided3(sd, gs, cfg, params.copy(), threads=4)["field"][5 + i]
    assert np.all(np.isfinite(ref)) and int(np.any(ref != 0, axis=1).sum()) == 37
    return ref


def test_3d_volumetric_points_with_a_frozen_network_match_the_oracle(oracle, frozen3):
    import torch
    gi = _gi3(oracle, _scene3(), 16, 16, 3, 4)
    p0 = gi.network.params()
    kw = dict(seed_base=5, seed_width=16, train_spp=0)
    field = gi.solve_points(_points3(), **kw)
    host_stats = dict(gi.last_stats)
    assert np.array_equal(field, frozen3), float(np.abs(field - frozen3).max())
    assert host_stats["optimizer_steps"] == 0 == host_stats["train_samples"] and host_stats["walks_started"] == 40 * 3
    assert np.array_equal(gi.network.params(), p0)
    # device arrays; a point that is not finite
    pts = torch.from_numpy(_points3()).cuda()
    out = torch.full((len(pts), 3), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stats = gi.solve_points_dev(pts.data_ptr(), len(pts), out.data_ptr(), **kw)
    assert np.array_equal(out.cpu().numpy(), frozen3)
    for k in COUNTERS:
        assert stats[k] == host_stats[k], k
    bad = _points3()
    bad[11, 0] = np.inf
    pts = torch.from_numpy(bad).cuda()
    out.fill_(-1.0)
    torch.cuda.synchronize()
    stats = gi.solve_points_dev(pts.data_ptr(), len(pts), out.data_ptr(), **kw)
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[11])) and np.array_equal(np.delete(got, 11, 0), np.delete(frozen3, 11, 0))
    assert stats["walks_started"] == host_stats["walks_started"] - 3
    from elaina_amd import capi
    with pytest.raises(capi.WostError, match="point 11 "):
        gi.solve_points(bad, **kw)
    with pytest.raises(capi.WostError, match="256"):
        gi.solve_points(np.full((257, 3), 0.5, np.float32), **kw)
    gi.close()
