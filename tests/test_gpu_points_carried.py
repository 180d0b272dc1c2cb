"""The carried point list (wost_points_carry & co., 2-D and 3-D) against the unchanged oracle, bit for bit.

A point of a bound list continues its own PCG32 stream and fp32 sums whenever a call takes it up, so after any sequence of calls
a point with n samples behind it holds the oracle's solve of that point at spp = n (test_gpu_points: a zero-scale probe at the
point, the single pixel seed_base + i), and the counters of a call are the oracle's on the selected points.  Fields are compared
with np.array_equal; the batch statistics with the numpy fp32 restatement of test_gpu_adaptive, fed with the sums read after
each call."""
import numpy as np
import pytest

from conftest import sphere_scene3, wiggly_problem
from test_gpu_adaptive import _Model, _assert_fields_by_count, _assert_state
from test_gpu_parity import _integrator
from test_gpu_points import (BOX, COUNTERS, _assert_points, _box_points, _cube_points, _it3, _mixed_box, _oracle_points, _wiggly_points,
                             box_ref, cube_ref)  # noqa: F401  (box_ref, cube_ref: fixtures)

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 96
BASE, WIDTH, DEPTH, EPS = BOX["seed_base"], BOX["seed_width"], BOX["depth"], BOX["eps"]
CALLS = ((2, "A"), (3, "B"), (1, None), (4, "AB"))


def _selections(n):
    """A: the first half of every run of 16 plus three single points of the other halves; B: a fixed-seed 30 %"""
    a = np.arange(n) % 16 < 8
    for i in (9, 44, 95):
        assert not a[i]
        a[i] = True
    b = np.random.default_rng(20261019).random(n) < 0.3
    assert (a & b).any() and (a & ~b).any() and (~a & b).any() and (~a & ~b).any()
    return {"A": a, "B": b, "AB": a & b, None: None}


def _box_refs(oracle, counts):
    """the oracle at the first 96 box points, one reference per sample count"""
    sd, pts = _mixed_box().as_dict(), _box_points()[:N]
    return {k: _oracle_points(oracle, "carried-box-%d" % k, sd, pts, BASE, WIDTH, k, DEPTH, EPS) for k in counts}


class _List:
    """the list of an integrator seen as _assert_state sees a frame"""

    def __init__(self, it):
        self.carried = it.points_carried


def _box_list(n=N, w=32, h=32, first=0):
    it = _integrator(_mixed_box(), w, h, 7, DEPTH, EPS)
    it.points_carry(_box_points()[first:first + n], BASE + first, WIDTH)
    return it


def _counters(stats):
    return {c: stats[c] for c in COUNTERS}


def _ref_counters(ref, rows, minus=None):
    return {c: int(ref[c][rows].sum()) - (int(minus[c][rows].sum()) if minus is not None else 0) for c in COUNTERS}


def _run_calls(it, calls, sels, n):
    """the calls on a list of n points -> the field after the last one"""
    field = None
    for more, name in calls:
        field = it.points_more(more, sels[name])
    return field


# ---- 1. calls on selections -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}],
                         ids=lambda o: "-".join("%s%d" % (k[:5], v) for k, v in o.items()) or "defaults")
def test_calls_on_selections_reproduce_the_oracle_at_every_points_own_count(oracle, opts):
    from elaina_amd import capi
    refs = _box_refs(oracle, (1, 2, 3, 4, 5, 6, 10))
    sels = _selections(N)
    it = _box_list()
    for k, v in opts.items():
        it.set_option(k, v)
    assert (it.n_points, it.points_done) == (N, 0)
    model, done = _Model(N), 0
    for i, (more, name) in enumerate(CALLS):
        sel = sels[name]
        field = it.points_more(more, sel)
        stats = dict(it.last_stats)
        done += more
        model.close_call(it.points_carried()["sum"], np.ones(N, bool) if sel is None else sel, more)
        print("call", i, name, _counters(stats), "counts", np.unique(model.n).tolist())
        _assert_fields_by_count(field, model.n, refs)
        _assert_state(_List(it), model, field)
        assert it.points_done == done
        if i == 0:
            assert _counters(stats) == _ref_counters(refs[2], sels["A"])
        if i == 3:
            assert _counters(stats) == _ref_counters(refs[10], sels["AB"], minus=refs[6])
        kinds = [l["kind"] for l in it.last_launches()]
        if opts.get("persist"):
            assert kinds[0] == capi.LAUNCH_PERSISTENT
        if opts.get("quad"):
            assert capi.LAUNCH_QUAD in kinds
    assert np.unique(model.n).tolist() == [1, 3, 4, 10]
    it.close()


# ---- 2. a list longer than the frame ----------------------------------------------------------------------------------------
def test_a_list_longer_than_the_frame_runs_in_chunks(oracle, box_ref):  # noqa: F811
    """an 8 x 8 frame holds 64 walkers: chunks of 64, 64, 64 and 8 points; a chunk in which nothing is selected walks nothing"""
    pts = _box_points()
    it = _integrator(_mixed_box(), 8, 8, 7, DEPTH, EPS)
    it.points_carry(pts, BASE, WIDTH)
    it.points_more(3)
    first = _counters(it.last_stats)
    field = it.points_more(5)
    assert np.array_equal(field, box_ref["field"])
    total = {c: first[c] + it.last_stats[c] for c in COUNTERS}
    assert total == _ref_counters(box_ref, slice(None)) and total["walk_steps"] == 26147 and total["walks_truncated"] == 329
    assert it.last_stats["kernel_launches"] >= 4
    ref12 = _oracle_points(oracle, "carried-box200-12", _mixed_box().as_dict(), pts, BASE, WIDTH, 12, DEPTH, EPS)
    sel = np.ones(200, bool)
    sel[64:128] = False
    field = it.points_more(4, sel)
    c = it.points_carried()
    assert np.array_equal(field[~sel], box_ref["field"][~sel]) and np.all(c["spp"][~sel] == 8) and np.all(c["batches"][~sel] == 2)
    assert np.array_equal(field[sel], ref12["field"][sel]) and np.all(c["spp"][sel] == 12) and np.all(c["batches"][sel] == 3)
    assert _counters(it.last_stats) == _ref_counters(ref12, sel, minus=box_ref)
    launches = it.last_launches()
    done = [l["walk_steps_done"] for l in launches if l["kind_name"] != "wait"]
    assert len(done) >= 3 and done == sorted(done) and 0 < done[-1] <= it.last_stats["walk_steps"]
    it.close()


# ---- 3. the smallest selections ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0, 95])
def test_one_point_and_an_empty_selection(oracle, index):
    refs = _box_refs(oracle, (3, 5))
    it = _box_list()
    one = np.zeros(N, bool)
    one[index] = True
    field = it.points_more(3, one)
    assert np.array_equal(field[index], refs[3]["field"][index]) and np.any(field[index] != 0) and np.all(field[~one] == 0.0)
    assert _counters(it.last_stats) == _ref_counters(refs[3], one)
    assert it.last_stats["kernel_launches"] > 0 and len(it.last_launches()) > 0
    c = it.points_carried()
    assert c["spp"][index] == 3 and c["batches"][index] == 1 and c["spp"].sum() == 3
    # nothing selected: nothing launched, the field of the state, no batch counted
    again = it.points_more(5, np.zeros(N, bool))
    assert all(it.last_stats[k] == 0 for k in COUNTERS) and it.last_stats["kernel_launches"] == 0 and it.last_launches() == []
    assert np.array_equal(again, field)
    c2 = it.points_carried()
    assert all(np.array_equal(c[k], c2[k], equal_nan=True) for k in c)
    assert it.points_done == 8
    # the point goes on from its own count
    field = it.points_more(2, one)
    assert np.array_equal(field[index], refs[5]["field"][index]) and it.points_carried()["batches"][index] == 2
    it.close()


def test_a_list_of_one_point(oracle):
    refs = _box_refs(oracle, (2, 5))
    it = _box_list(n=1)
    assert np.array_equal(it.points_more(2), refs[2]["field"][:1])
    assert _counters(it.last_stats) == _ref_counters(refs[2], slice(0, 1))
    assert np.array_equal(it.points_more(3), refs[5]["field"][:1])
    c = it.points_carried()
    assert c["spp"].tolist() == [5] and c["batches"].tolist() == [2] and np.all(np.isfinite(c["stderr"]))
    it.close()


# ---- 4. points that are not finite ------------------------------------------------------------------------------------------
def test_points_that_are_not_finite(oracle):
    import torch
    from elaina_amd import capi
    refs = _box_refs(oracle, (2, 5, 6))
    it = _box_list()
    it.points_more(2)
    before = it.points_carried()
    bad = _box_points()[:N].copy()
    bad[5, 1] = np.nan
    bad[70, 0] = np.inf
    # the host bind refuses the list and the one bound before stays
    with pytest.raises(capi.WostError, match="point 5 "):
        it.points_carry(bad, BASE, WIDTH)
    after = it.points_carried()
    assert it.n_points == N and all(np.array_equal(before[k], after[k], equal_nan=True) for k in before) and np.all(after["spp"] == 2)
    # the device bind takes it: the two points are never walked, never selected, and answer NaN
    stream = torch.cuda.current_stream().cuda_stream
    pts = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    it.points_carry_dev(pts.data_ptr(), N, stream, BASE, WIDTH)
    assert (it.n_points, it.points_done) == (N, 0) and not it.points_carried()["spp"].any()
    good = np.ones(N, bool)
    good[[5, 70]] = False
    field = torch.full((N, 3), -1.0, dtype=torch.float32, device="cuda")
    everyone = torch.ones(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    model = _Model(N)

    def check(walked, more):
        f = field.cpu().numpy()
        c = it.points_carried()
        model.close_call(c["sum"], walked, more)
        assert np.all(np.isnan(f[~good]))
        assert np.all(c["spp"][~good] == 0) and np.all(c["batches"][~good] == 0) and np.all(c["sum"][~good] == 0)
        assert np.all(np.isposinf(c["stderr"][~good]))
        assert np.array_equal(c["spp"], model.n) and np.array_equal(c["batches"], model.K)
        assert np.array_equal(c["stderr"], model.stderr(c["sum"]), equal_nan=True)
        _assert_fields_by_count(f[good], model.n[good], {k: {"field": r["field"][good]} for k, r in refs.items()})

    stats = it.points_more_dev(2, field.data_ptr(), None, stream)
    assert _counters(stats) == _ref_counters(refs[2], good)
    check(good, 2)
    stats = it.points_more_dev(3, field.data_ptr(), everyone.data_ptr(), stream)
    assert _counters(stats) == _ref_counters(refs[5], good, minus=refs[2])
    check(good, 3)
    assert np.all(model.n[good] == 5)
    # abs_tol 0: only a point without any variance (one on the Dirichlet boundary) is converged; every other finite point takes
    # the one batch there is room for, and the tolerance never selects the two that are not finite (their +inf is above it)
    want = model.selection(it.points_carried()["sum"], 1, 2, 6, 0.0, 0.0)
    assert want[~good].all() and want[good].sum() >= N // 2
    stats = it.points_adaptive_dev(1, 6, field.data_ptr(), stream, abs_tol=0.0, min_batches=2)
    assert _counters(stats) == _ref_counters(refs[6], want & good, minus=refs[5]) and stats["kernel_launches"] >= 1
    check(want & good, 1)
    it.close()


# ---- 5. far and strayed points ----------------------------------------------------------------------------------------------
def test_far_and_strayed_points_continue_from_their_carried_state(oracle):
    """the wave scan of the init on a carried start (two points hundreds of extents away) and walkers that stray"""
    p = wiggly_problem(emissive=True)
    pts = _wiggly_points()
    ref = _oracle_points(oracle, "wiggly", p.as_dict(), pts, 0, 16, 4, 16, 0.5)
    it = _integrator(p, 16, 16, 4, 16, 0.5)
    it.points_carry(pts, 0, 16)
    it.points_more(1)
    first = _counters(it.last_stats)
    field = it.points_more(3)
    _assert_points(field, {c: first[c] + it.last_stats[c] for c in COUNTERS}, ref)
    assert np.all(it.points_carried()["spp"] == 4)
    it.close()


# ---- 6. adaptive ------------------------------------------------------------------------------------------------------------
def _replay(it, model, n, batch_spp, min_batches, max_spp, abs_tol, rel_tol=0.0):
    """the adaptive loop by hand: points_more on the selection computed in numpy from points_carried() -> counters, selections"""
    total, sizes = dict.fromkeys(COUNTERS, 0), []
    while True:
        c = it.points_carried()
        assert np.array_equal(c["spp"], model.n) and np.array_equal(c["batches"], model.K)
        sel = model.selection(c["sum"], batch_spp, min_batches, max_spp, abs_tol, rel_tol)
        if not sel.any():
            return total, sizes
        it.points_more(batch_spp, sel)
        model.close_call(it.points_carried()["sum"], sel, batch_spp)
        sizes.append(int(sel.sum()))
        for k in COUNTERS:
            total[k] += it.last_stats[k]


def test_adaptive_solve_is_the_replayed_loop(oracle):
    """96 box points, batches of 4, min_batches 3, max_spp 48, abs_tol 0.2.  Simulated on the CPU from the oracle alone (sum ~
    field * n in float64, an approximation of the fp32 sums): 12 rounds on 96, 96, 96, 58, 45, 38, 30, 25, 22, 21, 18, 16 points,
    final counts on every multiple of 4 from 12 to 48, 38 points stop at 12, 16 reach the cap."""
    kw = dict(batch_spp=4, min_batches=3, max_spp=48, abs_tol=0.2)
    refs = _box_refs(oracle, tuple(range(4, 49, 4)))
    it = _box_list()
    field, se, n = it.points_adaptive(kw["batch_spp"], kw["max_spp"], abs_tol=kw["abs_tol"], min_batches=kw["min_batches"])
    stats, launches = dict(it.last_stats), it.last_launches()
    man, model = _box_list(), _Model(N)
    total, sizes = _replay(man, model, N, **kw)
    print("adaptive rounds", sizes, "counts", dict(zip(*np.unique(model.n, return_counts=True))))
    c = _assert_state(_List(man), model, man.points_more(1, np.zeros(N, bool)))
    state = it.points_carried()
    assert np.array_equal(n, model.n) and all(np.array_equal(state[k], c[k], equal_nan=True) for k in c)
    assert np.array_equal(se, c["stderr"])
    with np.errstate(all="ignore"):
        assert np.array_equal(field, c["sum"] / c["spp"].astype(f32)[:, None])
    assert _counters(stats) == total and stats["kernel_launches"] >= len(sizes) and it.points_done == 4 * len(sizes)
    done = [l["walk_steps_done"] for l in launches if l["kind_name"] != "wait"]
    assert len(done) >= len(sizes) and done == sorted(done) and stats["walk_steps"] // 2 < done[-1] <= stats["walk_steps"]
    _assert_fields_by_count(field, n, refs)
    # what keeps the test meaningful
    inner = np.unique(n[(n > 12) & (n < 48)])
    assert np.all(n % 4 == 0) and n.min() >= 12 and (n < 48).sum() >= 10 and (n == 48).sum() >= 5 and len(inner) >= 3
    # a second call with a tighter tolerance resumes
    field2, se2, n2 = it.points_adaptive(4, 48, abs_tol=0.12, min_batches=3)
    assert np.all(n2 >= n) and np.any(n2 > n) and n2.max() <= 48
    _assert_fields_by_count(field2, n2, refs)
    _replay(man, model, N, 4, 3, 48, 0.12)
    assert np.array_equal(n2, model.n) and np.array_equal(se2, man.points_carried()["stderr"])
    man.close()
    it.close()


# ---- 7. neighbours ----------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_the_list_and_the_carried_frame_leave_each_other_alone(oracle):
    refs = _box_refs(oracle, (2, 5))
    pts = _box_points()
    both, frame, only = _box_list(), _integrator(_mixed_box(), 32, 32, 7, DEPTH, EPS), _box_list()
    both.solve_more(2)
    both.points_more(3)
    both.solve()
    both.solve_points(pts[100:140], 3, 16)
    both.set_option("quad", 1)
    both.solve_more(1)
    list_field = both.points_more(1)
    frame.solve_more(2)
    frame.solve_more(1)
    only.points_more(3)
    assert np.array_equal(both.solution, frame.solution) and _same(both.carried(), frame.carried()) and both.spp_done == frame.spp_done == 3
    assert np.array_equal(list_field, only.points_more(1)) and _same(both.points_carried(), only.points_carried())
    assert both.points_done == only.points_done == 4
    # the two restarts
    state = both.points_carried()
    both.restart()
    assert _same(both.points_carried(), state) and both.points_done == 4 and not both.carried()["spp"].any()
    both.solve_more(2)
    frame_state = both.carried()
    both.points_restart()
    c = both.points_carried()
    assert not c["spp"].any() and not c["batches"].any() and not c["sum"].any() and np.all(np.isposinf(c["stderr"]))
    assert (both.n_points, both.points_done) == (N, 0) and _same(both.carried(), frame_state)
    assert np.array_equal(both.points_more(5), refs[5]["field"])
    # another list forgets the first
    both.points_carry(pts[40:N], BASE + 40, WIDTH)
    c = both.points_carried()
    assert (both.n_points, both.points_done) == (N - 40, 0) and len(c["spp"]) == N - 40 and not c["spp"].any()
    assert np.array_equal(both.points_more(2), refs[2]["field"][40:])
    # ... and an empty one releases it
    both.points_carry(np.zeros((0, 2), f32))
    assert both.n_points == 0
    from elaina_amd import capi
    with pytest.raises(capi.WostError, match="no point list is bound"):
        both.points_more(1)
    for it in (both, frame, only):
        it.close()


# ---- 8. cuts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [((2, None), (3, None)), CALLS], ids=["everyone", "selections"])
def test_a_cut_list_reproduces_the_uncut_one(calls):
    sels = _selections(N)
    whole = _box_list()
    want = _run_calls(whole, calls, sels, N)
    state = whole.points_carried()
    for first, n in ((0, 40), (40, 56)):
        rows = slice(first, first + n)
        part = _box_list(n=n, first=first)
        cut = {k: None if v is None else v[rows] for k, v in sels.items()}
        assert np.array_equal(_run_calls(part, calls, cut, n), want[rows])
        assert _same(part.points_carried(), {k: v[rows] for k, v in state.items()})
        part.close()
    whole.close()


# ---- 9. 3-D -----------------------------------------------------------------------------------------------------------------
N3 = 130


def _cube_refs(oracle, cube_ref):  # noqa: F811
    sd, ref4 = cube_ref
    refs = {k: _oracle_points(oracle, "carried-cube3-%d" % k, sd, _cube_points(), 5, 16, k, 32, 1e-3, dim=3) for k in (1, 2, 3)}
    refs[4] = ref4
    return sd, refs


def _cube_list(sd):
    it = _it3(sd, 16, 16, 6, 32, 1e-3)
    it.points_carry(_cube_points(), 5, 16)
    return it


def test_3d_calls_on_selections_and_the_state(oracle, cube_ref):  # noqa: F811
    import torch
    sd, refs = _cube_refs(oracle, cube_ref)
    sels = _selections(N3)
    a, b = sels["A"], sels["B"]
    it = _cube_list(sd)
    model = _Model(N3)
    for i, (more, sel) in enumerate(((1, None), (2, a), (1, b))):
        before = model.n.copy()
        field = it.points_more(more, sel)
        walked = np.ones(N3, bool) if sel is None else sel
        model.close_call(it.points_carried()["sum"], walked, more)
        _assert_fields_by_count(field, model.n, refs)
        _assert_state(_List(it), model, field)
        assert it.last_stats["kernel_launches"] == 1
        if i == 0:
            assert _counters(it.last_stats) == _ref_counters(refs[1], slice(None))
        if i == 2:
            want = dict.fromkeys(COUNTERS, 0)
            for k in np.unique(before[b]):
                rows = b & (before == k)
                step = _ref_counters(refs[int(k) + 1], rows, minus=refs[int(k)])
                want = {c: want[c] + step[c] for c in COUNTERS}
            assert _counters(it.last_stats) == want
    assert np.unique(model.n).tolist() == [1, 2, 3, 4] and it.points_done == 4
    it.close()
    # one point -- the one beyond huge2 -- and an empty selection
    it = _cube_list(sd)
    one = np.zeros(N3, bool)
    one[129] = True
    field = it.points_more(3, one)
    assert np.array_equal(field[129], refs[3]["field"][129]) and np.all(field[~one] == 0.0)
    assert _counters(it.last_stats) == _ref_counters(refs[3], one) and it.last_stats["kernel_launches"] == 1
    again = it.points_more(2, np.zeros(N3, bool))
    assert all(it.last_stats[k] == 0 for k in COUNTERS) and it.last_stats["kernel_launches"] == 0 and np.array_equal(again, field)
    assert np.array_equal(it.points_more(1, one)[129], refs[4]["field"][129]) and it.points_carried()["spp"].sum() == 4
    # the device forms on the caller's stream
    stream = torch.cuda.current_stream().cuda_stream
    pts = torch.from_numpy(_cube_points()).cuda()
    out = torch.full((N3, 3), -1.0, dtype=torch.float32, device="cuda")
    sel_dev = torch.from_numpy(a.astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    it.points_carry_dev(pts.data_ptr(), N3, stream, 5, 16)
    stats = it.points_more_dev(2, out.data_ptr(), None, stream)
    assert _counters(stats) == _ref_counters(refs[2], slice(None)) and np.array_equal(out.cpu().numpy(), refs[2]["field"])
    stats = it.points_more_dev(1, out.data_ptr(), sel_dev.data_ptr(), stream)
    assert _counters(stats) == _ref_counters(refs[3], a, minus=refs[2])
    assert np.array_equal(out.cpu().numpy(), np.where(a[:, None], refs[3]["field"], refs[2]["field"]))
    it.close()


def test_3d_the_frames_own_points_continue_to_the_frame_solve():
    sd = sphere_scene3(subdiv=2, value=lambda x, y, z: x + 0.5 * z, probe=(0.5, (0.0, 0.0, 0.25), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
    it = _it3(sd, 32, 32, 8, 32, 1e-3)
    it.solve()
    want, stats = it.solution.copy(), dict(it.last_stats)
    py, px = np.divmod(np.arange(32 * 32), 32)
    ndcx, ndcy = (2.0 * px / 32 - 1.0).astype(f32), (2.0 * py / 32 - 1.0).astype(f32)
    pts = np.stack([f32(0.5) * ndcx, f32(0.5) * ndcy, np.full(32 * 32, 0.25, f32)], 1).astype(f32)
    it.points_carry(pts, 0, 32)
    it.points_more(3)
    first = _counters(it.last_stats)
    field = it.points_more(5)
    assert {c: first[c] + it.last_stats[c] for c in COUNTERS} == {c: stats[c] for c in COUNTERS}
    assert np.any(want != 0) and np.array_equal(field, want)
    it.close()


# abs_tol of the 3-D adaptive run, chosen from the oracle alone so that both outcomes occur.  Simulated on the CPU from the
# oracle's fields at 2, 4, 6 and 8 spp (sum ~ field * n in float64): with 0.15 the rounds take 130, 130, 60 and 49 points, 70
# points stop at 4 samples, 11 at 6 and 49 reach the cap of 8 (0.05: 48 / 2 / 80; 0.3: 96 / 20 / 14).
ABS_TOL3 = 0.15


def test_3d_adaptive_solve_is_the_replayed_loop(oracle, cube_ref):  # noqa: F811
    sd, _ = cube_ref
    kw = dict(batch_spp=2, min_batches=2, max_spp=8, abs_tol=ABS_TOL3)
    refs = {k: _oracle_points(oracle, "carried-cube3-%d" % k, sd, _cube_points(), 5, 16, k, 32, 1e-3, dim=3) for k in (2, 6, 8)}
    refs[4] = cube_ref[1]
    it = _cube_list(sd)
    field, se, n = it.points_adaptive(kw["batch_spp"], kw["max_spp"], abs_tol=kw["abs_tol"], min_batches=kw["min_batches"])
    stats = dict(it.last_stats)
    man, model = _cube_list(sd), _Model(N3)
    total, sizes = _replay(man, model, N3, **kw)
    print("3-D adaptive rounds", sizes, "counts", dict(zip(*np.unique(model.n, return_counts=True))))
    c = _assert_state(_List(man), model, man.points_more(1, np.zeros(N3, bool)))
    assert np.array_equal(n, model.n) and _same(it.points_carried(), c) and np.array_equal(se, c["stderr"])
    assert _counters(stats) == total and stats["kernel_launches"] == len(sizes)
    _assert_fields_by_count(field, n, refs)
    # both outcomes: points that stop early, and points that reach the cap
    assert np.all(n % 2 == 0) and n.min() >= 4 and (n < 8).sum() >= 10 and (n == 8).sum() >= 10
    man.close()
    it.close()
