"""Continued uniform solves (wost_solve_more & co., 2-D and 3-D) against the unchanged oracle, bit for bit.

The oracle adds a pixel's samples to fp32 sums in order on one PCG32 stream and divides once at the end, so the field after
continued calls of a, b, c ... samples is the oracle's solve at spp = a, a + b, a + b + c ...; the counters of a call are the
differences of the oracle's cumulative ones.  Fields are compared with np.array_equal."""
import os
import subprocess

import numpy as np
import pytest

from conftest import box_problem, cube_scene3, sphere_scene3, wiggly_problem
from test_gpu_parity import THREADS, _cached_ref, _integrator, _with_source

pytestmark = pytest.mark.gpu

COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits")
_REFS = {}


def _refs(oracle, key, sd, w, h, cuts, depth, eps, dim=2):
    """the oracle's solves at the cumulative sample counts `cuts`, once per key: {spp: result}"""
    if key not in _REFS:
        solve = oracle.solve if dim == 2 else oracle.solve3
        _REFS[key] = {k: solve(sd, w, h, k, depth, eps, threads=THREADS) for k in cuts}
    return _REFS[key]


def _assert_call(field, stats, refs, done, before):
    """the field after a call that brought the solve to `done` samples, and the call's own counters"""
    ref = refs[done]
    print("spp_done", done, {c: stats[c] for c in COUNTERS})
    assert field.dtype == np.float32 and field.shape == ref["field"].shape
    assert np.array_equal(field, ref["field"]), (done, float(np.abs(field - ref["field"]).max()))
    for c in COUNTERS:
        assert stats[c] == ref[c] - (refs[before][c] if before else 0), (c, done, stats[c])


def _owned_by_shard(w, h, shard_index, shard_count):
    """the pixels of a shard: whole 8x8 tiles, (w + 7) / 8 of them per row, dealt round robin"""
    py, px = np.divmod(np.arange(w * h), w)
    return ((py >> 3) * ((w + 7) >> 3) + (px >> 3)) % shard_count == shard_index


def _more_sharded(it, w, h, shard_index, shard_count, more):
    """one continued call of a shard into a zero-filled device tensor of the whole frame -> the (n, 3) field"""
    import torch
    buf = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    it.solve_more_sharded(shard_index, shard_count, more, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(-1, 3)


# ---- 1. the ladybug frame --------------------------------------------------------------------------------------------------
LADY = dict(w=96, h=80, depth=64, eps=1.0, calls=(1, 1, 3, 11, 8), cuts=(1, 2, 5, 16, 24))


@pytest.fixture(scope="module")
def lady_refs(oracle, ladybug):
    # (3, 4 and 8 samples: the cuts of the shard and restart tests)
    refs = dict(_refs(oracle, "ladybug", ladybug.as_dict(), LADY["w"], LADY["h"], (1, 2, 3, 4, 5, 8, 16), LADY["depth"], LADY["eps"]))
    refs[24] = _cached_ref(oracle, ladybug, "persist-ladybug", 96, 80, 24, 64, 1.0)
    # the oracle's answers are what the issue recorded
    assert [refs[k]["walk_steps"] for k in LADY["cuts"]] == [55258, 111485, 277955, 889438, 1334577]
    assert [refs[k]["walks_truncated"] for k in LADY["cuts"]] == [2, 3, 7, 13, 18]
    # every cut is a different field: the pixels that change from one cut to the next (many of the ladybug's pixels see one flat
    # colour in their first samples, so fewer change at the first two cuts; 7 644 or more of the 7 680 at the later ones)
    assert all(np.all(np.isfinite(refs[k]["field"])) for k in LADY["cuts"])
    changed = [int(np.any(refs[a]["field"] != refs[b]["field"], axis=1).sum()) for a, b in zip(LADY["cuts"], LADY["cuts"][1:])]
    assert changed == [4859, 6808, 7665, 7644]
    return refs


@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"block_size": 64}],
                         ids=lambda o: "-".join("%s%d" % (k[:5], v) for k, v in o.items()) or "defaults")
def test_continued_calls_reproduce_the_oracle_at_every_cut(lady_refs, ladybug, opts):
    from elaina_amd import capi
    it = _integrator(ladybug, LADY["w"], LADY["h"], 7, LADY["depth"], LADY["eps"])
    for k, v in opts.items():
        it.set_option(k, v)
    assert it.spp_done == 0
    done = 0
    for more in LADY["calls"]:
        it.solve_more(more)
        _assert_call(it.solution, it.last_stats, lady_refs, done + more, done)
        done += more
        assert it.spp_done == done
        assert np.all(np.isfinite(it.solution))
        if opts.get("persist"):
            assert it.last_launches()[0]["kind"] == capi.LAUNCH_PERSISTENT
    # the handle's own setting was neither read nor changed
    it.solve()
    want = _integrator(ladybug, LADY["w"], LADY["h"], 7, LADY["depth"], LADY["eps"])
    want.solve()
    assert np.array_equal(it.solution, want.solution) and it.spp_done == done
    want.close()
    it.close()


def test_launch_options_may_change_between_the_calls(lady_refs, ladybug):
    from elaina_amd import capi
    it = _integrator(ladybug, LADY["w"], LADY["h"], 7, LADY["depth"], LADY["eps"])
    plans = [{"refill": 1}, {"refill": -1, "persist": 1, "resident_blocks": 1}, {"persist": -1, "resident_blocks": 0, "quad": 1},
             {"quad": -1, "block_size": 64}, {"block_size": 256}]
    done = 0
    for more, plan in zip(LADY["calls"], plans):
        for k, v in plan.items():
            it.set_option(k, v)
        it.solve_more(more)
        _assert_call(it.solution, it.last_stats, lady_refs, done + more, done)
        done += more
        kinds = [l["kind"] for l in it.last_launches()]
        if plan.get("refill") == 1:
            assert kinds[0] == capi.LAUNCH_ONE
        if plan.get("persist") == 1:
            assert kinds[0] == capi.LAUNCH_PERSISTENT
        if plan.get("quad") == 1:
            assert capi.LAUNCH_QUAD in kinds
    it.close()


# ---- 2. emissive boundary on the tree, strayed walkers ---------------------------------------------------------------------
def test_emissive_tree_scene_with_strayed_walkers(oracle):
    p = wiggly_problem(emissive=True)
    refs = _refs(oracle, "wiggly", p.as_dict(), 32, 32, (2, 3, 8), 16, 0.5)
    assert [refs[k]["walk_steps"] for k in (2, 3, 8)] == [30219, 45353, 120978]
    assert [refs[k]["walks_truncated"] for k in (2, 3, 8)] == [1738, 2599, 6929]
    it = _integrator(p, 32, 32, 5, 16, 0.5)
    done, strayed = 0, 0
    for more in (2, 1, 5):
        it.solve_more(more)
        _assert_call(it.solution, it.last_stats, refs, done + more, done)
        done += more
        assert np.all(np.isfinite(it.solution)) and np.all(np.any(it.solution != 0, axis=1))
        # (no persistent launch here: what ran beside an ordinary launch were the strayed walkers of the one before)
        launches = it.last_launches()
        assert all(l["kind"] != 3 for l in launches)
        strayed += sum(l["walkers_beside"] for l in launches)
    print("strayed walkers served", strayed)
    assert strayed > 0
    it.close()


# ---- 3. mixed boundaries, a mask, a source term ----------------------------------------------------------------------------
def _mixed_box(masked):
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: 1.0 + x + 2.0 * y, flux=lambda x, y, s: 0.3 * (s - 2))
    if masked:
        mask = np.ones((32, 32), np.uint8)
        mask[::3, 1::2] = 0
        p.mask = mask.reshape(-1)
    return p


def test_masked_pixels_stay_zero_and_carry_nothing(oracle):
    p = _mixed_box(True)
    off = p.mask == 0
    assert int(off.sum()) == 176
    refs = _refs(oracle, "box-mask", p.as_dict(), 32, 32, (1, 4, 9), 32, 1e-3)
    assert [refs[k]["walk_steps"] for k in (1, 4, 9)] == [10439, 40419, 90761]
    it = _integrator(p, 32, 32, 2, 32, 1e-3)
    done = 0
    for more in (1, 3, 5):
        it.solve_more(more)
        _assert_call(it.solution, it.last_stats, refs, done + more, done)
        done += more
        assert np.all(it.solution[off] == 0.0) and np.all(np.any(it.solution[~off] != 0, axis=1))
    it.close()


def test_source_term_under_a_persistent_launch(oracle):
    p = _with_source(_mixed_box(False), 0.0, 1.0)
    refs = _refs(oracle, "box-source", p.as_dict(), 32, 32, (2, 6), 32, 1e-3)
    it = _integrator(p, 32, 32, 3, 32, 1e-3)
    it.set_option("persist", 1)
    it.set_option("resident_blocks", 1)
    from elaina_amd import capi
    done = 0
    for more in (2, 4):
        it.solve_more(more)
        _assert_call(it.solution, it.last_stats, refs, done + more, done)
        done += more
        assert it.last_launches()[0]["kind"] == capi.LAUNCH_PERSISTENT
    it.close()


# ---- 4. shards -------------------------------------------------------------------------------------------------------------
def test_two_shards_carry_their_own_solves(lady_refs, ladybug):
    from elaina_amd import capi
    w, h = LADY["w"], LADY["h"]
    its = [_integrator(ladybug, w, h, 7, LADY["depth"], LADY["eps"]) for _ in range(2)]
    own = [_owned_by_shard(w, h, r, 2) for r in range(2)]
    done = 0
    for more in (3, 5):
        parts, stats = [], []
        for r, it in enumerate(its):
            parts.append(_more_sharded(it, w, h, r, 2, more))
            stats.append(dict(it.last_stats))
            assert np.all(parts[r][~own[r]] == 0.0), r
        total = {c: sum(s[c] for s in stats) for c in COUNTERS}
        _assert_call(parts[0] + parts[1], total, lady_refs, done + more, done)
        done += more
        assert [it.spp_done for it in its] == [done, done]
    # the carried solve of handle 0 belongs to shard 0 of 2
    with pytest.raises(capi.WostError, match="shard 0 of 2"):
        _more_sharded(its[0], w, h, 1, 2, 1)
    with pytest.raises(capi.WostError, match="shard 0 of 2"):
        its[0].solve_more(1)
    assert its[0].spp_done == 8
    its[0].restart()
    assert its[0].spp_done == 0
    part = _more_sharded(its[0], w, h, 1, 2, 3)
    ref3 = lady_refs[3]["field"]
    assert np.array_equal(part[own[1]], ref3[own[1]]) and np.all(part[~own[1]] == 0.0)
    for it in its:
        it.close()


# ---- 5. independence and refusals on a live handle -------------------------------------------------------------------------
def test_other_solves_and_refusals_leave_the_carried_solve_alone(lady_refs, ladybug):
    from elaina_amd import capi
    it = _integrator(ladybug, LADY["w"], LADY["h"], 7, LADY["depth"], LADY["eps"])
    it.solve_more(1)
    _assert_call(it.solution, it.last_stats, lady_refs, 1, 0)
    it.solve()
    it.solve_points(np.array([[100.0, 120.0], [250.0, 300.0], [400.0, 90.0]], np.float32), 5, 96)
    it.set_option("spp", 3)
    with pytest.raises(capi.WostError, match=r"2\^20-1"):
        it.solve_more((1 << 20) - 1)
    assert it.spp_done == 1
    it.solve_more(1)
    _assert_call(it.solution, it.last_stats, lady_refs, 2, 1)
    it.restart()
    assert it.spp_done == 0
    it.solve_more(4)
    ref4 = lady_refs[4]
    assert np.array_equal(it.solution, ref4["field"]) and it.last_stats["walk_steps"] == ref4["walk_steps"] and it.spp_done == 4
    it.close()


# ---- 6. 3-D ----------------------------------------------------------------------------------------------------------------
def _it3(sd, w, h, spp, depth, eps):
    from elaina_amd import UniformIntegratorSettings
    from elaina_amd.integrator3d import Problem3, UniformIntegrator3
    return UniformIntegrator3(Problem3.from_dict(sd), UniformIntegratorSettings((w, h), spp, depth, eps))


def _cube3():
    return cube_scene3(n=2, d_faces=(0, 1), n_faces=(2, 3, 4, 5), value=lambda x, y, z: x + z, flux=lambda x, y, z, f: 0.1 * (f - 3))


def _continue3(it, refs, calls):
    done = 0
    for more in calls:
        it.solve_more(more)
        _assert_call(it.solution, it.last_stats, refs, done + more, done)
        done += more
        assert it.spp_done == done


def test_3d_tiled_frame(oracle):
    sd = _cube3()
    refs = _refs(oracle, "cube3-tiled", sd, 24, 16, (1, 3, 4, 12), 48, 2e-3, dim=3)
    assert [refs[k]["walk_steps"] for k in (1, 3, 4, 12)] == [7217, 21979, 29094, 87018]
    for a, b in ((1, 3), (3, 4), (4, 12)):
        assert int(np.any(refs[a]["field"] != refs[b]["field"], axis=1).sum()) == 384
    it = _it3(sd, 24, 16, 6, 48, 2e-3)
    _continue3(it, refs, (1, 2, 1, 8))
    # the handle's own setting was neither read nor changed, and its solve leaves the carried one alone
    it.solve()
    six = oracle.solve3(sd, 24, 16, 6, 48, 2e-3, threads=THREADS)
    assert np.array_equal(it.solution, six["field"]) and it.spp_done == 12
    it.close()


def test_3d_untiled_frame(oracle):
    sd = _cube3()
    refs = _refs(oracle, "cube3-untiled", sd, 20, 12, (2, 5), 48, 2e-3, dim=3)
    it = _it3(sd, 20, 12, 6, 48, 2e-3)
    _continue3(it, refs, (2, 3))
    it.close()


def test_3d_two_shards(oracle):
    from elaina_amd import capi
    sd = _cube3()
    w, h = 24, 16
    refs = _refs(oracle, "cube3-shards", sd, w, h, (3, 8), 48, 2e-3, dim=3)
    its = [_it3(sd, w, h, 6, 48, 2e-3) for _ in range(2)]
    own = [_owned_by_shard(w, h, r, 2) for r in range(2)]
    done = 0
    for more in (3, 5):
        parts, stats = [], []
        for r, it in enumerate(its):
            parts.append(_more_sharded(it, w, h, r, 2, more))
            stats.append(dict(it.last_stats))
            assert np.all(parts[r][~own[r]] == 0.0), r
        _assert_call(parts[0] + parts[1], {c: sum(s[c] for s in stats) for c in COUNTERS}, refs, done + more, done)
        done += more
    with pytest.raises(capi.WostError, match="shard 1 of 2"):
        _more_sharded(its[1], w, h, 0, 2, 1)
    its[1].restart()
    part = _more_sharded(its[1], w, h, 0, 2, 3)
    assert np.array_equal(part[own[0]], refs[3]["field"][own[0]]) and np.all(part[~own[0]] == 0.0)
    for it in its:
        it.close()


@pytest.mark.parametrize("wave", ["0", "1"])
def test_3d_neumann_tree_scene(oracle, monkeypatch, wave):
    """a Dirichlet icosphere inside a 1280-triangle Neumann icosphere (the shell of tests/test_gpu_3d.py): the NTREE instantiations,
    with the closest-point queries by the lane and by the wave"""
    inner = sphere_scene3(subdiv=1, radius=0.45, value=lambda x, y, z: x)
    outer = sphere_scene3(subdiv=3, radius=1.0)
    sd = dict(inner)
    sd["n_verts"], sd["n_tris"], sd["n_colors"] = outer["d_verts"], outer["d_tris"], outer["d_colors"]
    sd["probe"] = (0.7, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))
    assert len(sd["n_tris"]) == 1280
    refs = _refs(oracle, "shell3", sd, 16, 16, (1, 3), 24, 1e-3, dim=3)
    monkeypatch.setenv("WOST3_WAVE", wave)
    it = _it3(sd, 16, 16, 2, 24, 1e-3)
    _continue3(it, refs, (1, 2))
    it.close()


# ---- 7. the host mirror ----------------------------------------------------------------------------------------------------
def test_host_3d_metric_frames_come_from_continued_solves(oracle, tmp_path):
    """saveSppMetrics* / saveTimeMetrics* of UniformIntegrator<3> through the C++ host: frame k holds the solution after k + 1
    samples (8-bit PNG quantisation applied), the last continued call is the solution"""
    import json
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import export_scene
    from test_host_exec import _exe, _read_png
    sd = cube_scene3(n=2, d_faces=(0, 1), n_faces=(2, 3, 4, 5), value=lambda x, y, z: x + z, flux=lambda x, y, z, f: 0.0)
    conf = export_scene.export3(sd, str(tmp_path), frame=(24, 16), spp=5, depth=48, eps=2e-3)
    c = json.load(open(conf))
    c["integrator"]["setting"].update({"saveSppMetricsDuration": 2, "saveSppMetricsUntil": 4, "saveTimeMetricsDuration": 4})
    json.dump(c, open(conf, "w"))
    out = subprocess.run([_exe(), conf], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exp = tmp_path / "exp" / "scene3d"
    assert sorted(os.listdir(exp / "frames")) == ["0.exr", "0.png", "2.exr", "2.png"]
    for k in (0, 2):
        ref = oracle.solve3(sd, 24, 16, k + 1, 48, 2e-3, threads=THREADS)["field"]
        png = _read_png(exp / "frames" / ("%d.png" % k))
        assert np.array_equal(png[::-1, :, :3].reshape(-1, 3), np.clip((ref * np.float32(255)).astype(np.int32), 0, 255))
    final = oracle.solve3(sd, 24, 16, 5, 48, 2e-3, threads=THREADS)
    assert np.array_equal(export_scene.read_pfm(exp / "solution.pfm"), final["field"])
    assert json.load(open(exp / "result.json"))["walk_steps"] == final["walk_steps"]
    names = os.listdir(exp / "frames_time")
    assert len(names) in (2, 4) and all(n_.split(".")[0].isdigit() for n_ in names)
