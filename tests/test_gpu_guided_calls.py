"""The front of the guided solve that the 2-D and the 3-D integrator share (solve, solve_sharded, the point solves, queryNetwork,
train_set), the same checks for both dimensions, bit for bit (np.array_equal throughout).

The references are the build's own: a second, equally seeded handle; the network's inference on inputs normalised in this file;
the field of an earlier call.  (The solves themselves are pinned to the oracle by test_guided_integrator.py, test_guided_3d.py and
test_gpu_guided_points.py.)  Frame 20 x 13 = 260 walkers: one full block of 256 and a ragged one; spp 4, two of them trained,
every third pixel from offset 2 a training pixel, fp32 network."""
import ctypes as C
import types

import numpy as np
import pytest

from conftest import box_problem, cube_scene3

pytestmark = pytest.mark.gpu

W, H, SPP, TRAIN_SPP, STRIDE, OFFSET = 20, 13, 4, 2, 3, 2
N = W * H
EPS = 1e-3
AABB = {2: ((-0.1, -0.1), (1.1, 1.1)), 3: ((-0.1, -0.1, -0.1), (1.1, 1.1, 1.1))}
COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits", "guided_steps", "train_samples", "optimizer_steps")


def _integrator(dim, train_spp=TRAIN_SPP):
    from elaina_amd.guided import GuidedIntegrator, GuidedIntegratorSettings
    from elaina_amd.integrator3d import GuidedIntegrator3, Problem3, default_net_config3
    st = GuidedIntegratorSettings(frameSize=(W, H), samplesPerPixel=SPP, trainSppCount=train_spp, maxWalkingDepth=32 if dim == 2 else 48,
                                  epsilonShell=EPS, batchSize=128, minBatchSize=128, trainPixelStride=STRIDE, trainPixelOffset=OFFSET)
    if dim == 2:
        # u(x, y) = y on the unit square: Dirichlet bottom / top, zero-flux Neumann left / right (test_guided_integrator.laplace_box)
        prob = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.0, n_per_side=8)
        return GuidedIntegrator(prob, st, AABB[2], seed=7)
    # the cube of test_gpu_guided_points._scene3, probed on the slice z = 0.5
    sd = cube_scene3(n=3, d_faces=(4, 5), n_faces=(0, 1, 2, 3), value=lambda x, y, z: z, flux=lambda x, y, z, f: 0.3 * (f - 1.5),
                     probe=(0.25, (0.5, 0.5, 0.5), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
    return GuidedIntegrator3(Problem3.from_dict(sd), st, AABB[3], network_config=default_net_config3(n_levels=4), seed=7)


def _points(dim, n, seed):
    return np.random.default_rng(seed).uniform(0.05, 0.95, (n, dim)).astype(np.float32)


@pytest.fixture(scope="module", params=[2, 3], ids=["2d", "3d"])
def solved(request):
    """per dimension, once: a.solve(), b.solve_sharded(0, 1) on an equally seeded handle, and c.solve() with one trained sample --
    its only training set is the first of a's two"""
    import torch
    dim = request.param
    a, b, c = _integrator(dim), _integrator(dim), _integrator(dim, train_spp=1)
    a.solve()
    dev = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    b.solve_sharded(0, 1, dev.data_ptr())
    c.solve()
    s = types.SimpleNamespace(dim=dim, a=a, b=b, c=c, a_stats=dict(a.last_stats), b_stats=dict(b.last_stats), c_stats=dict(c.last_stats),
                              sharded=dev.cpu().numpy(), dev=dev)
    yield s
    for gi in (a, b, c):
        gi.close()


# ---- solves, network and training set ------------------------------------------------------------------------------------------
def test_solve_and_one_shard_of_one_agree(solved):
    s = solved
    assert s.a.solution.shape == (N, 3) and np.all(np.isfinite(s.a.solution)) and np.any(s.a.solution != 0)
    assert np.array_equal(s.a.solution, s.sharded)
    for k in COUNTERS:
        assert s.a_stats[k] == s.b_stats[k], k
    assert s.a_stats["walks_started"] == SPP * N and s.a_stats["train_samples"] > 0 and s.a_stats["guided_steps"] > 0
    assert s.a_stats["reserved"] == OFFSET == s.b_stats["reserved"]


@pytest.mark.parametrize("index,count", [(0, 0), (-1, 1), (2, 2)])
def test_a_shard_outside_its_count_is_refused(solved, index, count):
    from elaina_amd import capi
    before = dict(solved.b.last_stats)
    with pytest.raises(capi.WostError, match="bad shard"):
        solved.b.solve_sharded(index, count, solved.dev.data_ptr())
    assert solved.b.last_stats == before


def _normalised(dim, p):
    """0.5 + (p - c) / e with centre and extent of the box inflated by 0.5 % of its diagonal, every step rounded to float32 in the
    order of the handle's constructor (the squares of the diagonal are added in order)"""
    f = np.float32
    lo, hi = np.array(AABB[dim][0], f), np.array(AABB[dim][1], f)
    d = hi - lo
    sq = d * d
    total = sq[0]
    for a in range(1, dim):
        total = f(total + sq[a])
    infl = f(np.sqrt(total) * f(0.005))
    blo, bhi = lo - infl, hi + infl
    c, e = (blo + bhi) / f(2.0), bhi - blo
    assert c.dtype == e.dtype == np.float32
    return f(0.5) + (p - c) / e


def test_query_network_is_the_inference_at_the_normalised_points(solved):
    """compared against network.inference on inputs normalised here in float32 (not against the second handle)"""
    s = solved
    p = np.concatenate([_points(s.dim, 37, 1), np.array([[-0.25] * s.dim, [1.5] * s.dim], np.float32)])
    x = _normalised(s.dim, p)
    assert x.dtype == np.float32
    raw = s.a.queryNetwork(p)
    assert raw.shape == (39, 33 if s.dim == 2 else 41) and np.all(np.isfinite(raw)) and np.any(raw != 0)
    assert np.array_equal(raw, s.a.network.inference(x))
    assert np.array_equal(s.a.queryNetwork(p[5]), raw[5])
    assert np.array_equal(raw, s.b.queryNetwork(p))


def test_the_training_set_is_the_last_pass_and_a_short_capacity_cuts_the_copy(solved):
    s = solved
    key = "xy" if s.dim == 2 else "xyz"
    ts, first = s.a.train_set(), s.c.train_set()
    m = len(ts[key])
    # a's two training passes: the first is c's only one (the walk of sample 0 sees the untrained network in both)
    assert s.c_stats["train_samples"] == len(first[key]) > 0
    assert m > 0 and len(first[key]) + m == s.a_stats["train_samples"]
    assert set(ts) == {key, "dir", "solution", "dir_pdf", "normal", "on_neumann"} and all(len(v) == m for v in ts.values())
    assert ts[key].shape == (m, s.dim) and np.all(np.isfinite(ts[key])) and np.all((ts[key] > 0) & (ts[key] < 1))
    other = s.b.train_set()
    for k in ts:
        assert np.array_equal(ts[k], other[k]), k
    # capacity m // 2: *n is still m, the arrays are written up to the capacity only
    from elaina_amd import capi
    fn = getattr(s.a.lib, ("wost_guided_" if s.dim == 2 else "wost3_guided_") + "train_set")
    half, n = m // 2, C.c_int32(-1)
    out = {k: np.full(v.shape, 77, v.dtype) for k, v in ts.items()}
    rc = fn(s.a._handle, half, C.byref(n), capi._fp(out[key]), capi._fp(out["dir"]), capi._fp(out["solution"]), capi._fp(out["dir_pdf"]),
            capi._fp(out["normal"]), out["on_neumann"].ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0 and n.value == m
    for k in ts:
        assert np.array_equal(out[k][:half], ts[k][:half]), k
        assert np.all(out[k][half:] == 77), k


# ---- point solves (train_spp = 0: the network does not move) --------------------------------------------------------------------
def test_point_lists_grow_and_reuse_the_handles_buffer(solved):
    import torch
    s = solved
    p0 = s.a.network.params()
    few, many = _points(s.dim, 8, 2), _points(s.dim, 200, 3)
    first = s.a.solve_points(few, train_spp=0)
    first_stats = dict(s.a.last_stats)
    assert first.shape == (8, 3) and np.all(np.isfinite(first)) and np.any(first != 0)
    assert first_stats["walks_started"] == 8 * SPP and first_stats["train_samples"] == 0 == first_stats["optimizer_steps"]
    grown = s.a.solve_points(many, train_spp=0)
    assert grown.shape == (200, 3) and s.a.last_stats["walks_started"] == 200 * SPP
    assert np.all(np.isfinite(grown)) and np.any(grown != 0)
    third = s.a.solve_points(few, train_spp=0)
    assert np.array_equal(first, third)
    for k in COUNTERS:
        assert s.a.last_stats[k] == first_stats[k], k
    # the same list from device memory
    pts = torch.from_numpy(few).cuda()
    field = torch.full((8, 3), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stats = s.a.solve_points_dev(pts.data_ptr(), 8, field.data_ptr(), train_spp=0)
    assert np.array_equal(field.cpu().numpy(), first)
    for k in COUNTERS:
        assert stats[k] == first_stats[k], k
    # a NaN coordinate: a NaN entry, its neighbours as they were
    bad = few.copy()
    bad[3, s.dim - 1] = np.nan
    pts = torch.from_numpy(bad).cuda()
    field.fill_(-1.0)
    torch.cuda.synchronize()
    stats = s.a.solve_points_dev(pts.data_ptr(), 8, field.data_ptr(), train_spp=0)
    got = field.cpu().numpy()
    assert np.all(np.isnan(got[3])) and np.array_equal(np.delete(got, 3, 0), np.delete(first, 3, 0))
    assert stats["walks_started"] == 7 * SPP
    assert np.array_equal(s.a.network.params(), p0)


def test_a_list_longer_than_the_frame_is_refused(solved):
    from elaina_amd import capi
    s = solved
    with pytest.raises(capi.WostError, match=r"width \* height = 260 points per call \(the handle's capacity\); got 261"):
        s.a.solve_points(np.full((N + 1, s.dim), 0.5, np.float32), train_spp=0)
    assert s.a.solve_points(np.full((N, s.dim), 0.5, np.float32), train_spp=0).shape == (N, 3)
