"""GPU parity tests: the HIP path, called through the C-ABI, against the CPU oracle on the
same seeded inputs.  Bar: bit-exact (fp32 field, integer counters, indices)."""
import os

import numpy as np
import pytest

from conftest import box_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden", "oracle_golden.npz")
THREADS = os.cpu_count() or 8


def _integrator(problem, w, h, spp, depth, eps):
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    return UniformIntegrator(problem, UniformIntegratorSettings((w, h), spp, depth, eps))


def _assert_same_solve(oracle, problem, w, h, spp, depth, eps, ref=None, **opts):
    """ref: the oracle's solve of these very arguments from an earlier call (the oracle has no options: one solve serves
    every variant of the HIP side)"""
    it = _integrator(problem, w, h, spp, depth, eps)
    for k, v in opts.items():
        it.set_option(k, v)
    it.solve()
    if ref is None:
        ref = oracle.solve(problem.as_dict(), w, h, spp, depth, eps, threads=THREADS)
    s = it.last_stats
    assert s["walk_steps"] == ref["walk_steps"]
    for k in ("walks_started", "walks_absorbed", "walks_truncated", "neumann_hits"):
        assert s[k] == ref[k], k
    assert np.array_equal(it.solution, ref["field"]), float(np.abs(it.solution - ref["field"]).max())
    it.close()
    return ref


@pytest.mark.parametrize("scene", ["ladybug", "fille"])
def test_closest_point_matches_golden_brute_force(scene):
    from elaina_amd import Problem
    g = np.load(GOLD)
    p = Problem.load_scene(scene)
    it = _integrator(p, 16, 16, 1, 4, 1.0)
    idx, dist, uv, side = it.closest_point(g[scene + "_cp_pts"])
    assert np.array_equal(idx, g[scene + "_cp_idx"])
    assert np.array_equal(dist, g[scene + "_cp_dist"])
    assert np.array_equal(uv, g[scene + "_cp_uv"])
    assert np.array_equal(side, g[scene + "_cp_side"].astype(np.int32))
    it.close()


def test_closest_point_random_mesh_and_ties(oracle):
    from elaina_amd import Problem
    rng = np.random.default_rng(2)
    n = 5000
    a = rng.uniform(0, 100, size=(n, 2))
    verts = np.concatenate([a, a + rng.normal(0, 1, size=(n, 2))]).astype(np.float32)
    segs = np.stack([np.arange(n), np.arange(n) + n], 1).astype(np.int32)
    # duplicate 500 segments so exact ties occur; lowest original index must win
    segs = np.concatenate([segs, segs[:500]])
    p = Problem(d_verts=verts, d_segs=segs)
    it = _integrator(p, 16, 16, 1, 4, 1.0)
    pts = rng.uniform(-20, 120, size=(100000, 2)).astype(np.float32)
    pts[::1000] *= 50.0                       # far outside the bounding box of the mesh
    got = it.closest_point(pts)
    ref = oracle.closest_point(verts, segs, pts, mode=1)
    for x, y in zip(got, ref):
        assert np.array_equal(x, y)
    it.close()


@pytest.mark.parametrize("n_segs", [1, 3, 4, 5, 16, 17, 64, 65, 257])
def test_closest_point_tiny_meshes(oracle, n_segs):
    # tree shapes around the leaf-size / arity boundaries, including padded (empty) leaves
    from elaina_amd import Problem
    rng = np.random.default_rng(n_segs)
    verts = rng.uniform(0, 10, size=(n_segs + 1, 2)).astype(np.float32)
    segs = np.stack([np.arange(n_segs), np.arange(n_segs) + 1], 1).astype(np.int32)
    it = _integrator(Problem(d_verts=verts, d_segs=segs), 16, 16, 1, 4, 1.0)
    pts = rng.uniform(-5, 15, size=(4096, 2)).astype(np.float32)
    got = it.closest_point(pts)
    ref = oracle.closest_point(verts, segs, pts, mode=0)
    for x, y in zip(got, ref):
        assert np.array_equal(x, y)
    it.close()


def test_silhouette_and_ray_queries(oracle, ladybug):
    it = _integrator(ladybug, 16, 16, 1, 4, 1.0)
    rng = np.random.default_rng(4)
    pts = rng.uniform(-400, 900, size=(20000, 2)).astype(np.float32)
    assert np.array_equal(it.closest_silhouette(pts), oracle.closest_silhouette(ladybug.n_verts, ladybug.n_segs, pts))
    rmax = rng.uniform(10, 600, size=20000).astype(np.float32)
    assert np.array_equal(it.closest_silhouette(pts, rmax),
                          oracle.closest_silhouette(ladybug.n_verts, ladybug.n_segs, pts, rmax))
    o = rng.uniform(-89, 589, size=(20000, 2)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, size=20000)
    d = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    tmax = rng.uniform(1, 900, size=20000).astype(np.float32)
    got = it.ray_intersect(o, d, tmax)
    ref = oracle.ray_intersect(ladybug.n_verts, ladybug.n_segs, o, d, tmax)
    assert np.array_equal(got[0], ref[0])
    hit = ref[0] == 1
    assert np.array_equal(got[1][hit], ref[1][hit]) and np.array_equal(got[2][hit], ref[2][hit])
    it.close()


def test_sdf_channels(oracle, ladybug):
    it = _integrator(ladybug, 64, 64, 1, 4, 1.0)
    assert np.array_equal(it.renderDirichletSDF(), oracle.render_dirichlet_sdf(ladybug.as_dict(), 64, 64, THREADS))
    assert np.all(np.isinf(it.renderSilhouetteSDF()))
    it.close()


def test_closest_point_exact_ties_between_parallel_segments(oracle):
    # two rows of 40 collinear horizontal segments: a point midway is at EXACTLY the same distance
    # from segments of different leaves, and duplicates tie inside a leaf; lowest original index wins
    from elaina_amd import Problem
    xs = np.arange(41, dtype=np.float32)
    verts = np.concatenate([np.stack([xs, np.zeros(41, np.float32)], 1), np.stack([xs, np.full(41, 2.0, np.float32)], 1)])
    segs = np.concatenate([np.stack([np.arange(40), np.arange(40) + 1], 1), np.stack([np.arange(40) + 41, np.arange(40) + 42], 1)])
    segs = np.concatenate([segs[::-1], segs[:16]]).astype(np.int32)        # reversed order + duplicates
    it = _integrator(Problem(d_verts=verts, d_segs=segs), 16, 16, 1, 4, 1.0)
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(-3, 43, 20000), np.ones(20000)], 1).astype(np.float32)       # y = 1: midway
    pts[10000:, 1] = rng.uniform(-2, 4, 10000).astype(np.float32)
    pts[::7, 0] = np.round(pts[::7, 0])                                                       # above shared vertices
    got = it.closest_point(pts)
    ref = oracle.closest_point(verts, segs, pts, mode=1)
    for x, y in zip(got, ref):
        assert np.array_equal(x, y)
    it.close()


@pytest.mark.parametrize("scene", ["ladybug", "fille"])
def test_config1_field_is_bit_exact_vs_golden(scene):
    # BASELINE.json configs[0]: 128^2, 16 spp, max_depth 32, eps 1
    from elaina_amd import Problem
    g = np.load(GOLD)
    it = _integrator(Problem.load_scene(scene), 128, 128, 16, 32, 1.0)
    it.solve()
    counts = g[scene + "_cfg1_counts"]
    s = it.last_stats
    assert [s["walk_steps"], s["walks_started"], s["walks_absorbed"], s["walks_truncated"], s["neumann_hits"]] == \
        [int(c) for c in counts]
    assert np.array_equal(it.solution, g[scene + "_cfg1_field"])
    it.close()


_REF_CACHE = {}


def _cached_ref(oracle, problem, key, *args):
    """one oracle solve per set of arguments for the parametrized variant tests below (the HIP side changes, the oracle's
    answer does not)"""
    if key not in _REF_CACHE:
        _REF_CACHE[key] = oracle.solve(problem.as_dict(), *args, threads=THREADS)
    return _REF_CACHE[key]


@pytest.mark.parametrize("steps_per_round", [1, 7, 64, 4096, 32767])
def test_round_length_does_not_change_results(oracle, ladybug, steps_per_round):
    _assert_same_solve(oracle, ladybug, 48, 40, 6, 24, 1.0, ref=_cached_ref(oracle, ladybug, "round", 48, 40, 6, 24, 1.0), steps_per_round=steps_per_round)


@pytest.mark.parametrize("opts", [
    {"wait_weight": 1}, {"wait_weight": 64}, {"trav_burst": 1}, {"trav_burst": 7},
])
def test_kernel_variants_do_not_change_results(oracle, ladybug, opts):
    # the scheduler knobs of the round kernel: same bits, same counters
    _assert_same_solve(oracle, ladybug, 56, 48, 6, 32, 1.0, ref=_cached_ref(oracle, ladybug, "variants", 56, 48, 6, 32, 1.0), **opts)


def test_ground_truth_sample_count(oracle, ladybug):
    """the reference's ground-truth configuration runs 65 536 samples per pixel (data/ladybug/gt.json): a pixel's sample
    counter, the per-launch 16-bit statistics and hundreds of rounds, on a frame (5 x 4) the oracle finishes in seconds"""
    ref = _assert_same_solve(oracle, ladybug, 5, 4, 65536, 64, 1.0)
    assert ref["walks_started"] == 20 * 65536


@pytest.mark.parametrize("block_size", [64, 128, 256])
def test_block_size_does_not_change_results(oracle, ladybug, block_size):
    _assert_same_solve(oracle, ladybug, 40, 48, 5, 24, 1.0, block_size=block_size)


@pytest.mark.parametrize("thin", [0, 1])
def test_thin_wave_launches_do_not_change_results(oracle, ladybug, thin):
    # 96 x 96 walkers fill < 1/16 of the chip: with thin_waves every launch gives one walker to
    # 2^k lanes; a pure scheduling choice
    _assert_same_solve(oracle, ladybug, 96, 96, 3, 32, 1.0, thin_waves=thin)


def test_ragged_frame_mask_and_ranges(oracle, ladybug):
    from elaina_amd import Problem
    w, h = 37, 29  # not a multiple of the 8x8 tile
    mask = (np.random.default_rng(0).uniform(size=w * h) > 0.3).astype(np.uint8)
    p = Problem(d_verts=ladybug.d_verts, d_segs=ladybug.d_segs, d_colors=ladybug.d_colors, n_verts=ladybug.n_verts,
                n_segs=ladybug.n_segs, probe=ladybug.probe, mask=mask)
    ref = _assert_same_solve(oracle, p, w, h, 5, 32, 1.0)
    assert np.all(ref["field"][mask == 0] == 0)
    it = _integrator(p, w, h, 5, 32, 1.0)
    parts = []
    for b, e in ((0, 1), (1, 500), (500, 500), (500, w * h)):
        it.solve(b, e)
        parts.append(it.solution.copy())
    assert np.array_equal(np.concatenate(parts), ref["field"])
    it.close()


def test_edge_settings(oracle, ladybug):
    _assert_same_solve(oracle, ladybug, 32, 32, 1, 1, 1.0)      # one step per walk
    _assert_same_solve(oracle, ladybug, 32, 32, 3, 200, 0.01)   # thin shell, long walks
    _assert_same_solve(oracle, ladybug, 8, 8, 40, 64, 5.0)      # fat shell


def test_dirichlet_only_and_neumann_only(oracle, ladybug):
    from elaina_amd import Problem
    d_only = Problem(d_verts=ladybug.d_verts, d_segs=ladybug.d_segs, d_colors=ladybug.d_colors, probe=ladybug.probe)
    _assert_same_solve(oracle, d_only, 32, 32, 4, 32, 1.0)
    # no Dirichlet boundary and no silhouette: R_B is infinite, every walk is dropped at depth 0
    n_only = Problem(n_verts=ladybug.n_verts, n_segs=ladybug.n_segs, probe=ladybug.probe)
    ref = _assert_same_solve(oracle, n_only, 16, 16, 3, 8, 1.0)
    assert ref["walk_steps"] == 16 * 16 * 3 and np.all(ref["field"] == 0)


def test_emissive_neumann_boundary(oracle):
    # non-zero Neumann colours exercise sample_object_in_sphere / shadow ray / Green's function
    flux = lambda x, y, side: -1.0 if side == 2 else 1.0
    p = box_problem(0.0, 100.0, 25, d_sides=(1, 3), n_sides=(0, 2), value=lambda x, y: y, flux=flux,
                    probe=(40.0, 50.0, 50.0, 0.0, 1.0))
    _assert_same_solve(oracle, p, 16, 16, 64, 512, 0.25)


def test_sharded_solve_sums_to_full_field(oracle, ladybug):
    import torch
    w, h, spp, depth = 64, 48, 4, 32
    ref = oracle.solve(ladybug.as_dict(), w, h, spp, depth, 1.0, threads=THREADS)
    it = _integrator(ladybug, w, h, spp, depth, 1.0)
    total = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    steps = 0
    for r in range(3):
        buf = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = it.solve_sharded(r, 3, buf.data_ptr())
        steps += st["walk_steps"]
        total += buf
    assert steps == ref["walk_steps"]
    assert np.array_equal(total.cpu().numpy().reshape(-1, 3), ref["field"])
    it.close()


def test_full_size_properties(oracle, ladybug):
    # BASELINE.json configs[1] frame (1024^2, depth 64) at 2 spp: size-independent properties
    w = h = 1024
    spp = 2
    it = _integrator(ladybug, w, h, spp, 64, 1.0)
    it.solve()
    s = it.last_stats
    f = it.solution
    assert s["walks_started"] == w * h * spp
    assert s["walks_absorbed"] + s["walks_truncated"] == s["walks_started"]
    assert np.isfinite(f).all() and f.min() >= 0.0 and f.max() <= 1.0
    # a band of rows against the oracle, bit for bit
    b, e = 500 * w, 508 * w
    ref = oracle.solve(ladybug.as_dict(), w, h, spp, 64, 1.0, pixel_begin=b, pixel_end=e, threads=THREADS)
    assert np.array_equal(f[b:e], ref["field"])
    # same launch twice: identical (no dependence on atomic ordering)
    it.solve()
    assert np.array_equal(it.solution, f) and it.last_stats["walk_steps"] == s["walk_steps"]
    it.close()


def test_constant_colour_counts_absorptions_exactly(ladybug):
    from elaina_amd import Problem
    p = Problem(d_verts=ladybug.d_verts, d_segs=ladybug.d_segs, d_colors=np.ones_like(ladybug.d_colors),
                n_verts=ladybug.n_verts, n_segs=ladybug.n_segs, probe=ladybug.probe)
    spp = 16
    it = _integrator(p, 256, 256, spp, 64, 1.0)
    it.solve()
    f = it.solution * spp
    assert np.array_equal(f, np.round(f))
    assert int(f[:, 0].sum()) == it.last_stats["walks_absorbed"]
    it.close()


def test_invalid_arguments_are_rejected(ladybug):
    from elaina_amd import UniformIntegratorSettings, UniformIntegrator, capi
    it = _integrator(ladybug, 16, 16, 1, 4, 1.0)
    with pytest.raises(capi.WostError):
        it.solve(-1, 10)
    with pytest.raises(capi.WostError):
        it.solve(0, 16 * 16 + 1)
    with pytest.raises(capi.WostError):
        it.set_option("no_such_option", 1)
    it.close()
    with pytest.raises(capi.WostError):
        UniformIntegrator(ladybug, UniformIntegratorSettings((0, 16), 1, 4, 1.0))


# ---- boundary meshes too large for the flat loops: LBVH + SNCH cone path ------------------
@pytest.mark.parametrize("open_gap", [0, 7])
def test_large_neumann_mesh_silhouette_and_ray_queries(oracle, open_gap):
    from conftest import wiggly_problem
    p = wiggly_problem(3000, 64, open_gap=open_gap)
    it = _integrator(p, 16, 16, 1, 4, 1.0)
    rng = np.random.default_rng(8)
    pts = rng.uniform(-140, 140, size=(20000, 2)).astype(np.float32)
    ref = oracle.closest_silhouette(p.n_verts, p.n_segs, pts)
    got = it.closest_silhouette(pts)
    assert np.isfinite(ref).mean() > 0.3          # the wiggly boundary does have silhouettes
    assert np.array_equal(got, ref)
    rmax = rng.uniform(1, 60, size=20000).astype(np.float32)
    assert np.array_equal(it.closest_silhouette(pts, rmax), oracle.closest_silhouette(p.n_verts, p.n_segs, pts, rmax))
    o = rng.uniform(-70, 70, size=(20000, 2)).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, size=20000)
    d = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    tmax = rng.uniform(1, 300, size=20000).astype(np.float32)
    gh, gt, gi = it.ray_intersect(o, d, tmax)
    rh, rt, ri = oracle.ray_intersect(p.n_verts, p.n_segs, o, d, tmax)
    assert np.array_equal(gh, rh) and rh.mean() > 0.2
    hit = rh == 1
    assert np.array_equal(gt[hit], rt[hit]) and np.array_equal(gi[hit], ri[hit])
    it.close()


def test_fine_neumann_mesh_rays_that_start_on_the_boundary(oracle):
    """30 000 segments of length 0.02 at |x| ~ 100: the node records are rounded images of the segments, several 10^-6 off the
    end points the exact test runs on -- more than the relative widening of the ray / box test allowed before round 3: rays that
    start on the boundary (a walker that has just hit it) were missed by the box of the very segment they stand on (630 of
    200 000 such rays; found by tools/probes/bench2d_coop.py with N_NEUMANN=30000).  Queries and a whole solve against the
    flat loops of the oracle."""
    from conftest import wiggly_problem
    p = wiggly_problem(30000, 64)
    it = _integrator(p, 16, 16, 1, 4, 1.0)
    rng = np.random.default_rng(9)
    n = 60000
    V, S = p.n_verts, p.n_segs
    si = rng.integers(0, len(S), n)
    a, b = V[S[si, 0]], V[S[si, 1]]
    on = (a + (b - a) * rng.uniform(0, 1, (n, 1)).astype(np.float32)).astype(np.float32)
    e = b - a
    nrm = np.stack([e[:, 1], -e[:, 0]], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = (on + rng.choice([0.0, 0.0, 0.05, -0.05, 1e-3, -1e-3], n)[:, None].astype(np.float32) * nrm).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, size=n)
    d = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
    tmax = (rng.uniform(0.5, 1.0, n) * rng.choice([0.03, 0.5, 10.0], n)).astype(np.float32)
    gh, gt, gi = it.ray_intersect(pts, d, tmax)
    rh, rt, ri = oracle.ray_intersect(V, S, pts, d, tmax)
    assert np.array_equal(gh, rh) and 0.1 < rh.mean() < 0.95
    hit = rh == 1
    assert np.array_equal(gt[hit], rt[hit]) and np.array_equal(gi[hit], ri[hit])
    assert np.array_equal(it.closest_silhouette(pts, np.full(n, 0.5, np.float32)), oracle.closest_silhouette(V, S, pts, np.full(n, 0.5, np.float32)))
    it.close()
    ref = _assert_same_solve(oracle, wiggly_problem(30000, 400), 48, 48, 4, 64, 0.05)
    _assert_same_solve(oracle, wiggly_problem(30000, 400), 48, 48, 4, 64, 0.05, ref=ref, coop=0)


@pytest.mark.parametrize("opts", [{}, {"refill": 1}])
def test_large_neumann_mesh_solve(oracle, opts):
    from conftest import wiggly_problem
    p = wiggly_problem(3000, 400)
    ref = _assert_same_solve(oracle, p, 24, 20, 6, 96, 0.5, **opts)
    assert ref["neumann_hits"] > 100


def test_large_emissive_neumann_mesh_solve(oracle):
    from conftest import wiggly_problem
    p = wiggly_problem(600, 200, emissive=True, open_gap=3)
    _assert_same_solve(oracle, p, 12, 10, 4, 64, 0.5)


def _run_bench(cmd, timeout=900):
    import json
    import subprocess
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_bench_two_ranks_sharing_one_gpu():
    # the N > 1 path of bench.py end to end (tile sharding + reduce + JSON contract) with two
    # processes on the one GPU of the test box under an EXTERNAL launcher (what the driver does);
    # gloo carries the reduce because RCCL refuses two ranks on one device
    import socket
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
           "--warmup", "0", "--frame", "128", "--spp", "8", "--backend", "gloo", "--full"]
    r = _run_bench(cmd)
    assert r["n_gpus"] == 2 and r["world_size"] == 2 and r["backend"] == "gloo"
    assert r["metric"] == "walk-steps/s" and r["scaling"] == "strong"
    assert r["rel_l2_vs_oracle"] == 0.0                       # the assembled field, checked against the oracle
    assert r["roofline"]["kernel"] == "walk_round_kernel" and "cpu_baseline" not in r     # host baseline: N = 1 only


def test_bench_starts_its_own_ranks():
    # `python bench.py --gpus 2` WITHOUT a launcher: bench.py itself starts the two ranks (a child
    # job spawned before the parent touches the GPU) and relays rank 0's line
    import sys
    env_clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    import json
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--frame", "128", "--spp", "8", "--backend", "gloo", "--full"], capture_output=True, text=True, timeout=900,
                         cwd=ROOT, env=env_clean)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["n_gpus"] == 2 and r["world_size"] == 2 and r["rel_l2_vs_oracle"] == 0.0


def test_bench_guided_config_two_ranks():
    # --config 4 scaled down, two self-started ranks on one GPU: the guided integrator through the
    # file the driver runs, shards + reduce, the MFMA fraction of the inference launches
    import json
    import subprocess
    import sys
    env_clean = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "4", "--gpus", "2", "--steps", "1", "--warmup",
                          "0", "--frame", "256", "--spp", "6", "--train-spp", "3", "--backend", "gloo", "--full"], capture_output=True,
                         text=True, timeout=900, cwd=ROOT, env=env_clean)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["n_gpus"] == 2 and r["config"]["config"] == 4 and r["field_finite"]
    # (the fused solve launches no network kernel of its own: the matrix-core figure is a probe and its key says so)
    mf = r.get("roofline_mfma") or r["mfma_probe_of_net_forward_kernel"]
    assert r["guided"]["guided_steps_per_pass"] > 0 and mf["bound"] == "mfma" and mf["achieved"] > 0
    assert r["roofline"]["kernel"] == "guided_sample_kernel" and r["guided"]["training_step"]["achieved"] > 0


@pytest.mark.parametrize("scene,spp,depth", [("ladybug", 1, 64), ("ladybug", 5, 32), ("fille", 2, 128)])
def test_refill_launch_matches_oracle(oracle, scene, spp, depth):
    """the single-launch path for few samples per pixel (lanes drain the input queue instead of
    waiting for a compaction): same per-pixel arithmetic, so still bit-exact"""
    from elaina_amd import Problem
    p = Problem.load_scene(scene)
    _assert_same_solve(oracle, p, 96, 80, spp, depth, 1.0, refill=1, block_size=64)
    _assert_same_solve(oracle, p, 96, 80, spp, depth, 1.0, refill=1)


def test_refill_launch_with_mask_and_mixed_boundaries(oracle):
    from conftest import box_problem, wiggly_problem
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.3 * (s - 2))
    mask = (np.arange(70 * 50) % 3 != 0).astype(np.uint8)
    p.mask = mask
    ref = _assert_same_solve(oracle, p, 70, 50, 3, 32, 1e-3, refill=1)
    assert np.all(ref["field"][mask == 0] == 0)
    _assert_same_solve(oracle, wiggly_problem(emissive=True), 48, 48, 2, 24, 0.05, refill=1)


def test_refill_is_chosen_automatically_for_one_sample(ladybug):
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    it = UniformIntegrator(ladybug, UniformIntegratorSettings((1024, 1024), 1, 64, 1.0))
    it.solve()
    assert it.last_stats["kernel_launches"] == 1
    ref = it.solution.copy()
    it.set_option("refill", 0)
    it.solve()
    assert it.last_stats["kernel_launches"] > 1 or it.last_stats["kernel_launches"] == 1
    assert np.array_equal(ref, it.solution)
    it.close()


@pytest.mark.parametrize("opts", [{"coop": 0}, {"coop": 1}, {"coop": 1, "pool_cap": 96}, {"coop": 1, "pool_cap": 200, "ray_slot_trigger": 1},
                                  {"coop": 1, "refill": 1}, {"coop": 1, "wait_weight": 8, "trav_burst": 1, "steps_per_round": 5}])
def test_neumann_tree_queries_by_the_wave_match_oracle(oracle, opts):
    """a Neumann mesh on the tree: the silhouette and ray queries of a step answered by the wave through its LDS task pools
    (wost_coop.h: closest_silhouette_wave, ray_closest_wave, step_finish_wave -- the default) against the per-lane descents;
    pools so small that the waves answer the old way (96 tasks: the 64 roots leave room for ten node tasks), slot tasks served
    one by one, the REFILL launch, short rounds.  Closed and open boundaries (open ends are silhouettes), emissive or not, with a
    source term: the oracle's field and counters."""
    from conftest import wiggly_problem
    _assert_same_solve(oracle, wiggly_problem(3000, 64, open_gap=0), 40, 40, 2, 24, 0.05, **opts)
    _assert_same_solve(oracle, wiggly_problem(3000, 64, open_gap=37), 40, 40, 2, 24, 0.05, **opts)
    _assert_same_solve(oracle, wiggly_problem(600, 200, emissive=True, open_gap=3), 32, 32, 3, 16, 0.05, **opts)
    _assert_same_solve(oracle, _with_source(wiggly_problem(emissive=True), -130.0, 130.0, intensity=1e-3), 32, 32, 2, 16, 0.05, **opts)


def test_quad_rounds_match_oracle(oracle, ladybug, fille):
    """walk_quad_kernel -- four lanes per walker, the descent shared between the lanes of a quad (wost_quad.h): the launch
    of an under-filled round.  Forced for every round here; same arithmetic per child, same keys and visiting order, so
    field and counters stay bit-exact: shipped scenes, exact ties, mixed boundaries with a mask, a 3000-segment emissive
    Neumann boundary on the tree, a source term, strayed walkers (open boundary seen from afar), short rounds."""
    from conftest import box_problem, wiggly_problem
    from elaina_amd import Problem
    _assert_same_solve(oracle, ladybug, 96, 80, 5, 64, 1.0, quad=1)
    _assert_same_solve(oracle, fille, 64, 48, 3, 128, 1.0, quad=1, steps_per_round=7, block_size=64)
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.3 * (s - 2))
    p.mask = (np.arange(70 * 50) % 3 != 0).astype(np.uint8)
    _assert_same_solve(oracle, p, 70, 50, 3, 32, 1e-3, quad=1, wait_weight=1, trav_burst=1)
    _assert_same_solve(oracle, wiggly_problem(emissive=True), 48, 48, 2, 24, 0.05, quad=1)
    _assert_same_solve(oracle, _with_source(wiggly_problem(emissive=False), -130.0, 130.0, intensity=1e-3), 40, 40, 2, 24, 0.05, quad=1)
    # two rows of collinear segments: exact ties between leaves and inside a leaf
    xs = np.arange(41, dtype=np.float32)
    verts = np.concatenate([np.stack([xs, np.zeros(41, np.float32)], 1), np.stack([xs, np.full(41, 2.0, np.float32)], 1)])
    segs = np.concatenate([np.stack([np.arange(40), np.arange(40) + 1], 1), np.stack([np.arange(40) + 41, np.arange(40) + 42], 1)])
    segs = np.concatenate([segs, segs[5:25]]).astype(np.int32)
    cols = np.random.default_rng(3).uniform(0, 1, (82, 6)).astype(np.float32)
    tie = Problem(d_verts=verts, d_segs=segs, d_colors=cols, probe=(30.0, 20.0, 1.0, 0.0, 1.0))
    _assert_same_solve(oracle, tie, 64, 64, 4, 16, 0.05, quad=1)
    # an open polyline seen from three scene sizes away: most walks stray and finish in the slack launch
    t = np.linspace(0.0, 1.0, 301)
    ov = np.stack([100.0 * t, 20.0 * np.sin(9.0 * t)], 1).astype(np.float32)
    os_ = np.stack([np.arange(300), np.arange(300) + 1], 1).astype(np.int32)
    far = Problem(d_verts=ov, d_segs=os_, d_colors=cols[:1].repeat(301, 0), probe=(300.0, 50.0, 0.0, 0.0, 1.0))
    _assert_same_solve(oracle, far, 64, 64, 3, 12, 0.5, quad=1)


def test_quad_rounds_are_chosen_for_under_filled_launches(ladybug):
    """automatic choice: the last rounds of a solve and a small shard run four lanes per walker; the field does not change"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    it = UniformIntegrator(ladybug, UniformIntegratorSettings((512, 512), 32, 64, 1.0))
    it.set_option("quad", 0)
    it.solve()
    a, sa = it.solution.copy(), dict(it.last_stats)
    it.set_option("quad", -1)
    it.solve()
    assert np.array_equal(a, it.solution) and it.last_stats["walk_steps"] == sa["walk_steps"]
    it.set_option("quad", 1)
    it.solve()
    assert np.array_equal(a, it.solution) and it.last_stats["walk_steps"] == sa["walk_steps"]
    it.close()


def test_refill_launch_open_scene_every_walk_strays(oracle):
    """An open Dirichlet polyline seen from three scene sizes away, 1024^2 at 1 spp (the automatic REFILL launch with a
    queue of 2.7 residencies): almost every walk strays beyond the plain visits' range at depth 1.  A resident lane whose
    walker strays hands it to the slack launch at once and goes on draining the queue; parked, the lanes stranded the
    unread pixels of the frame (round-2 advisor finding).  Every pixel must be solved: counters, then a band against the
    oracle bit for bit."""
    from elaina_amd import Problem, UniformIntegrator, UniformIntegratorSettings
    t = np.linspace(0.0, 1.0, 301)
    verts = np.stack([100.0 * t, 20.0 * np.sin(9.0 * t) + 5.0 * np.cos(31.0 * t)], 1).astype(np.float32)
    segs = np.stack([np.arange(300), np.arange(300) + 1], 1).astype(np.int32)
    rng = np.random.default_rng(5)
    cols = rng.uniform(0.0, 1.0, size=(301, 6)).astype(np.float32)
    p = Problem(d_verts=verts, d_segs=segs, d_colors=cols, probe=(300.0, 50.0, 0.0, 0.0, 1.0))
    W = 1024
    it = UniformIntegrator(p, UniformIntegratorSettings((W, W), 1, 12, 0.5))
    it.solve()
    s, a = dict(it.last_stats), it.solution.copy()
    assert s["walks_started"] == W * W == s["walks_absorbed"] + s["walks_truncated"]
    it.set_option("refill", 0)
    it.solve()
    assert it.last_stats["walks_started"] == W * W and it.last_stats["walk_steps"] == s["walk_steps"]
    assert np.array_equal(a, it.solution)
    it.close()
    b, e = 500 * W, 524 * W
    ref = oracle.solve(p.as_dict(), W, W, 1, 12, 0.5, pixel_begin=b, pixel_end=e, threads=THREADS)
    assert np.array_equal(a[b:e], ref["field"])
    assert np.isfinite(a).all()


@pytest.mark.parametrize("scene,spp,depth,opts", [
    ("ladybug", 24, 64, {"resident_blocks": 2}), ("ladybug", 24, 64, {"resident_blocks": 3, "block_size": 64}),
    ("ladybug", 24, 64, {"resident_blocks": 5, "persist_order": 0}), ("ladybug", 24, 64, {}),
    ("fille", 9, 128, {"resident_blocks": 4, "steps_per_round": 16}), ("fille", 9, 128, {"resident_blocks": 1, "quad": 1}),
    # what the persistent launch hands over: the longest remainders beside the rounds (every pixel, none, a capped number), the rest sorted or not
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 8}), ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 64, "long_cap": 37}),
    ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 0, "tail_sort": 0}), ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 48, "tail_sort": 0}),
    ("fille", 9, 128, {"resident_blocks": 8, "long_steps": 40, "steps_per_round": 8}),
    ("fille", 9, 128, {"resident_blocks": 8, "long_steps": 16, "long_thin": 5}), ("ladybug", 24, 64, {"resident_blocks": 6, "long_steps": 8, "long_thin": 0}),
])
def test_persistent_first_launch_matches_oracle(oracle, scene, spp, depth, opts):
    """The persistent first launch of a many-sample solve (round 6): a few resident blocks take the pixels of the frame one by
    one, longest expected chain first, and when none is unread every wave hands the pixels it holds -- mid-pixel, mid-walk --
    to the rounds.  A pixel's arithmetic does not depend on the lane that runs it or on where a launch ends: same bits, same
    counters (the steps in flight when the queue runs dry are counted once)."""
    from elaina_amd import Problem
    p = Problem.load_scene(scene)
    _assert_same_solve(oracle, p, 96, 80, spp, depth, 1.0, ref=_cached_ref(oracle, p, "persist-" + scene, 96, 80, spp, depth, 1.0), persist=1, **opts)


def test_persistent_first_launch_with_mask_mixed_boundaries_and_strays(oracle):
    from conftest import box_problem, wiggly_problem
    from elaina_amd import Problem
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.3 * (s - 2))
    mask = (np.arange(70 * 50) % 3 != 0).astype(np.uint8)
    p.mask = mask
    ref = _assert_same_solve(oracle, p, 70, 50, 12, 32, 1e-3, persist=1, resident_blocks=2)
    assert np.all(ref["field"][mask == 0] == 0)
    _assert_same_solve(oracle, wiggly_problem(emissive=True), 48, 48, 7, 24, 0.05, persist=1, resident_blocks=3)
    # an open polyline seen from afar: most walks stray beyond the plain visits' range, and a resident lane hands a strayed walker
    # to the slack launch and takes the next pixel
    t = np.linspace(0.0, 1.0, 301)
    verts = np.stack([100.0 * t, 20.0 * np.sin(9.0 * t) + 5.0 * np.cos(31.0 * t)], 1).astype(np.float32)
    segs = np.stack([np.arange(300), np.arange(300) + 1], 1).astype(np.int32)
    cols = np.random.default_rng(5).uniform(0.0, 1.0, size=(301, 6)).astype(np.float32)
    q = Problem(d_verts=verts, d_segs=segs, d_colors=cols, probe=(300.0, 50.0, 0.0, 0.0, 1.0))
    _assert_same_solve(oracle, q, 64, 64, 6, 12, 0.5, persist=1, resident_blocks=2)


def test_persistent_first_launch_is_chosen_for_a_full_frame_of_many_samples(ladybug):
    """1024^2 walkers on 393 216 resident lanes, 16 samples each: the automatic choice is one persistent launch plus the rounds of
    what it leaves; with persist = 0 the solve runs in rounds only.  Same field, same counters."""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    it = UniformIntegrator(ladybug, UniformIntegratorSettings((1024, 1024), 16, 64, 1.0))
    it.solve()
    a, sa = it.solution.copy(), dict(it.last_stats)
    it.set_option("persist", 0)
    it.solve()
    sb = dict(it.last_stats)
    assert np.array_equal(a, it.solution)
    # (not the node visits: the long remainders run with the visits that are exact at any distance, which prune a little less)
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits"):
        assert sa[k] == sb[k], k
    assert sa["walks_started"] == 16 * 1024 * 1024
    # the launches of the two solves as wost_last_launches reports them: rounds only now; before, one persistent launch that took
    # most of the steps, then rounds (and a wait for what ran beside them); the steps of the launches add up to the solve's
    from elaina_amd import capi
    rounds_only = it.last_launches()
    assert all(l["kind"] in (capi.LAUNCH_ROUND, capi.LAUNCH_QUAD) for l in rounds_only)
    assert rounds_only[-1]["walk_steps_done"] == sb["walk_steps"]
    it.set_option("persist", -1)
    it.solve()
    ll = it.last_launches()
    assert ll[0]["kind"] == capi.LAUNCH_PERSISTENT and ll[0]["walkers"] == 1024 * 1024 and ll[0]["steps"] > 0.5 * sa["walk_steps"]
    assert all(l["kind"] != capi.LAUNCH_PERSISTENT for l in ll[1:])
    assert sum(l.get("steps", 0) for l in ll) <= sa["walk_steps"]          # (what ran beside the last round ends inside the wait)
    assert len([l for l in ll if l["kind"] != capi.LAUNCH_WAIT]) == it.last_stats["kernel_launches"]
    it.close()


def _with_source(problem, lo, hi, cells=24, seed=9, intensity=0.7):
    """attach a smooth random RGB source grid covering [lo, hi]^2 (and a margin of zero outside)"""
    rng = np.random.default_rng(seed)
    n = cells + 1
    gx, gy = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n))
    rgb = np.stack([np.sin(3 * gx + 2 * gy) + 0.3 * rng.normal(size=gx.shape), gx * gy, 1.0 - gy], -1).astype(np.float32)
    s = cells / (hi - lo)
    problem.source = {"rgb": rgb, "index_scale": (s, s), "index_offset": (-lo * s, -lo * s), "intensity": intensity}
    return problem


def test_source_term_matches_oracle(oracle, ladybug):
    """sampleSource in the walk step: variable draw count per step (rejection
    sampler), Neumann clipping of the source ray, bilinear grid sampling -- bit-exact"""
    import copy
    from conftest import box_problem, wiggly_problem
    from test_oracle_solver import _poisson_disc
    _assert_same_solve(oracle, _poisson_disc(), 40, 36, 6, 48, 1e-3)
    mixed = _with_source(box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.2), 0.0, 1.0)
    _assert_same_solve(oracle, mixed, 48, 40, 5, 32, 1e-3)
    _assert_same_solve(oracle, mixed, 48, 40, 5, 32, 1e-3, steps_per_round=3, block_size=64)
    lb = _with_source(copy.copy(ladybug), -100.0, 600.0, cells=40, intensity=1e-3)
    _assert_same_solve(oracle, lb, 64, 48, 3, 64, 1.0)
    _assert_same_solve(oracle, _with_source(wiggly_problem(emissive=True), -130.0, 130.0, intensity=1e-3), 40, 40, 2, 24, 0.05)
    # the persistent first launch with a source term (round 6): a few resident blocks take the pixels, the hand-over with long remainders
    _assert_same_solve(oracle, mixed, 48, 40, 14, 32, 1e-3, persist=1, resident_blocks=2, long_steps=16)
    _assert_same_solve(oracle, lb, 64, 48, 9, 64, 1.0, persist=1, resident_blocks=3, block_size=64)
    _assert_same_solve(oracle, _with_source(wiggly_problem(emissive=True), -130.0, 130.0, intensity=1e-3), 40, 40, 7, 24, 0.05, persist=1, resident_blocks=2, long_steps=8)


def test_render_source_matches_oracle(oracle):
    from test_oracle_solver import _poisson_disc
    p = _with_source(_poisson_disc(), -0.8, 0.9, cells=7)
    p.probe = np.asarray((1.3, 0.1, -0.2, 0.6, 0.8), np.float32)
    it = _integrator(p, 37, 21, 1, 4, 1e-3)
    assert np.array_equal(it.renderSource(), oracle.render_source(p.as_dict(), 37, 21))
    it.close()
    p.source = None
    it = _integrator(p, 8, 8, 1, 4, 1e-3)
    assert np.all(it.renderSource() == 0)
    it.close()


def test_full_size_properties_config2(oracle, ladybug):
    """BASELINE config 2 at its full size (1024^2, 256 spp): an 8-row band bit-exact against the oracle,
    reproducibility, exact linearity in a power-of-two intensity, shard union, counter identities"""
    import copy
    import torch
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    st = UniformIntegratorSettings((1024, 1024), 256, 64, 1.0)
    it = UniformIntegrator(ladybug, st)
    it.solve()
    a, sa = it.solution.copy(), dict(it.last_stats)
    it.solve()
    assert np.array_equal(a, it.solution) and it.last_stats["walk_steps"] == sa["walk_steps"]
    # the band against the oracle: the 8 rows (of the 128 bands that start on a multiple of 8) with the largest mean
    # Dirichlet distance at this frame -- the longest chains, the pixels the persistent launch hands over to the
    # long-remainder launch.  For the ladybug that is rows 1016 .. 1023.
    band = int(np.argmax(it.renderDirichletSDF().reshape(128, 8 * 1024).mean(axis=1)))
    it.close()
    b, e = band * 8 * 1024, (band + 1) * 8 * 1024
    ref = oracle.solve(ladybug.as_dict(), 1024, 1024, 256, 64, 1.0, pixel_begin=b, pixel_end=e, threads=16)
    assert np.array_equal(a[b:e], ref["field"]), (band, float(np.abs(a[b:e] - ref["field"]).max()))
    assert sa["walks_started"] == 1024 * 1024 * 256 == sa["walks_absorbed"] + sa["walks_truncated"]
    assert sa["walk_steps"] == 1949024384          # the count every run of this configuration must reproduce
    assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0 + 1e-6      # convex combinations of colours in [0, 1]
    # doubling the Dirichlet intensity doubles every fp32 contribution exactly
    p2 = copy.copy(ladybug)
    p2.dirichlet_intensity = 2.0
    it = UniformIntegrator(p2, st)
    it.solve()
    assert np.array_equal(it.solution, 2.0 * a)
    it.close()
    # three shards written into device buffers sum to the same field
    total = torch.zeros(1024 * 1024 * 3, device="cuda")
    it = UniformIntegrator(ladybug, st)
    for r in range(3):
        buf = torch.zeros(1024 * 1024 * 3, device="cuda")
        it.solve_sharded(r, 3, buf.data_ptr())
        torch.cuda.synchronize()
        total += buf
    it.close()
    assert np.array_equal(total.cpu().numpy().reshape(-1, 3), a)


def test_full_size_config3_fille_band_and_properties(oracle, fille):
    """BASELINE config 3 at its full size (fille, 1024^2, 256 spp, depth 128: mixed boundary, one LBVH level
    deeper than ladybug) through the default round kernel: an 8-row band bit-exact against the oracle,
    reproducibility, counter identities and the walk-step count every run must reproduce"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    it = UniformIntegrator(fille, UniformIntegratorSettings((1024, 1024), 256, 128, 1.0))
    it.solve()
    a, sa = it.solution.copy(), dict(it.last_stats)
    it.solve()
    assert np.array_equal(a, it.solution) and it.last_stats["walk_steps"] == sa["walk_steps"] == 2467318167
    it.close()
    assert sa["walks_started"] == 1024 * 1024 * 256 == sa["walks_absorbed"] + sa["walks_truncated"]
    assert np.isfinite(a).all()
    b, e = 508 * 1024, 516 * 1024
    ref = oracle.solve(fille.as_dict(), 1024, 1024, 256, 128, 1.0, pixel_begin=b, pixel_end=e, threads=THREADS)
    assert np.array_equal(a[b:e], ref["field"])


@pytest.mark.parametrize("first", [0, 40, 80])
def test_random_scenes_match_the_oracle(first):
    """tools/fuzz/fuzz_parity.py: random closed and open polylines of 3 .. 2000 segments on either boundary kind, emissive
    or not, degenerate and doubled segments, scales from 1e-3 to 1e4, probes that look at the scene from 50 scene sizes away,
    source terms, the REFILL launch.  Found: closest points that differed from brute force far outside the mesh (HIP tree and
    the oracle's BVH alike -- walkers that stray that far leave the ordinary launch now and finish their walk in the kernel whose
    node visits carry a relative slack) and silhouette cones that pruned queries within the test's absolute precision of a
    vertex in scenes of that size."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz", "fuzz_parity.py"), str(first), "40"], capture_output=True,
                         text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "fuzz %d..%d: 0 mismatches" % (first, first + 39) in out.stdout, out.stdout[-3000:]
