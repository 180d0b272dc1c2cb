"""The carried gradient list (wost_gradient_points_carry & co.) against the single gradient call, which this list
leaves as it was: a batch of round r is a row of solve_gradient_points at the round's seeds on an integrator with spp = S, bit
for bit, and the list's outputs are those rows combined in numpy float64 in round order.

Tolerances, all derived and none measured: grad = (float)(G / K) and field = (float)(F / K) are sums and one division of exactly
representable numbers in fp64, hence equal bit for bit; Q - G G / K loses up to 2 ulp(Q) (the division and the subtraction; a
contracted multiply-add would be inside that), a relative 2 * 2^-53 * Q / v of v, of which the square root keeps half, and the
rounding to fp32 adds 2^-24."""
import numpy as np
import pytest

from test_gpu_gradient import ANALYTIC, BOX, LIN, _box_it, _box_points, _mixed_cube
from test_gpu_parity import _integrator, _with_source
from test_gpu_points import _it3, _mixed_box

pytestmark = pytest.mark.gpu

S = BOX["S"]
N, STRIDE = 70, 96                 # three blocks of 32 points, the last partial; the seeds of a round lie 96 apart
KEYS = ("grad", "stderr", "field", "radius", "batches")
WOST_ERR_INVALID, WOST_ERR_UNSUPPORTED = -1, -3


def _bind(it, pts, max_rounds, stride=STRIDE, seed_base=BOX["seed_base"], walk_seed_base=BOX["walk_seed_base"], batch_walks=S):
    it.gradient_points_carry(pts, batch_walks, stride, max_rounds, seed_base, walk_seed_base, BOX["seed_width"])


def _rows(ref, pts, rounds, stride=STRIDE, seed_base=BOX["seed_base"], walk_seed_base=BOX["walk_seed_base"], width=BOX["seed_width"], batch_walks=S):
    """the single call at the seeds of rounds 0 .. rounds - 1, on an integrator whose spp is the list's S"""
    return [ref.solve_gradient_points(pts, seed_base + r * stride, walk_seed_base + r * stride * batch_walks, width) for r in range(rounds)]


def _walkable(row, eps):
    R = row["radius"]
    return np.isfinite(R) & (R > np.float32(eps))


def _combine(rows, masks, walkable):
    """the state after the rounds whose single-call rows are `rows`, round r on the points of masks[r] (None: all)"""
    n, dim = rows[0]["grad"].shape[:2]
    G, Q, F, K = np.zeros((n, dim, 3)), np.zeros((n, dim, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
    for row, m in zip(rows, masks):
        w = walkable if m is None else walkable & (np.asarray(m) != 0)
        g = row["grad"].astype(np.float64)
        G[w] += g[w]
        Q[w] += g[w] * g[w]
        F[w] += row["field"].astype(np.float64)[w]
        K[w] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        Kd = K.astype(np.float64)[:, None, None]
        v = np.maximum(Q - G * G / Kd, 0.0)
        se = np.sqrt(v / ((Kd - 1.0) * Kd))
        se[K < 2] = np.inf
        se[~walkable] = np.nan
        return {"grad": (G / Kd).astype(np.float32), "field": (F / Kd[:, :, 0]).astype(np.float32), "se": se, "Q": Q, "v": v, "batches": K,
                "radius": rows[0]["radius"], "walkable": walkable}


def _assert_state(out, exp):
    K, walkable = exp["batches"], exp["walkable"]
    assert np.array_equal(out["batches"], K)
    assert np.array_equal(out["radius"], exp["radius"], equal_nan=True)
    assert np.array_equal(out["grad"], exp["grad"], equal_nan=True)
    assert np.array_equal(out["field"], exp["field"], equal_nan=True)
    assert np.all(K[~walkable] == 0) and np.all(np.isnan(out["grad"][~walkable])) and np.all(np.isnan(out["field"][~walkable]))
    assert np.all(np.isnan(out["stderr"][~walkable]))
    assert np.all(np.isposinf(out["stderr"][walkable & (K < 2)]))
    full = walkable & (K >= 2)
    se, got, Q, v = exp["se"][full], out["stderr"][full].astype(np.float64), exp["Q"][full], exp["v"][full]
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = np.where(v > 0.0, 2.0 ** -24 + 2.0 * 2.0 ** -53 * Q / v, 0.0)
    assert np.all(np.abs(got - se) <= bound * se), float(np.max(np.abs(got - se) / np.maximum(se, 1e-300)))


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def _third(n):
    return (np.arange(n) % 3 == 0).astype(np.uint8)


# ---- 1. a batch is a row of the single call -----------------------------------------------------------------------------------
def test_a_batch_is_a_row_of_the_single_call():
    pts = _box_points()[:N]
    middle = np.zeros(N, np.uint8)
    middle[32:64] = 1                       # blocks 0 and 2 launch nothing
    masks = [np.ones(N, np.uint8), _third(N), middle, None]
    ref = _box_it()
    rows = _rows(ref, pts, 4)
    ref.close()
    walkable = _walkable(rows[0], BOX["eps"])
    assert not walkable[0] and not walkable[1] and walkable[2] and walkable[3]
    it = _box_it()
    it.set_option("spp", 3)                 # the handle's spp is neither read nor changed
    _bind(it, pts, 5)
    assert it.gradient_points_done == (N, 0)
    launches = []
    for r, m in enumerate(masks):
        out = it.gradient_points_more(m)
        exp = _combine(rows[:r + 1], masks[:r + 1], walkable)
        _assert_state(out, exp)
        walked = int((walkable if m is None else walkable & (m != 0)).sum())
        assert it.last_stats["walks_started"] == S * walked, (r, it.last_stats)
        launches.append(it.last_stats["kernel_launches"])
        assert it.gradient_points_done == (N, r + 1)
        assert _same(out, it.gradient_points_carried())
    assert launches[2] < launches[0]        # one block of three walked
    assert np.all(np.isnan(out["grad"][:2])) and np.all(out["batches"][:2] == 0) and np.array_equal(out["radius"][:2], rows[0]["radius"][:2])
    # an empty selection: no round, zeroed stats, the state's outputs
    none = it.gradient_points_more(np.zeros(N, np.uint8))
    assert _same(none, out) and it.gradient_points_done == (N, 4)
    assert all(v == 0 for v in it.last_stats.values()), it.last_stats
    it.close()


# ---- 2. the cut and the neighbours -----------------------------------------------------------------------------------------------
def _three_rounds(it, second):
    """every point, the points of `second`, every point"""
    it.gradient_points_more()
    it.gradient_points_more(second)
    return it.gradient_points_more()


def test_a_cut_list_gives_the_same_bits_and_the_neighbours_change_nothing():
    pts = _box_points()[:N]
    it = _box_it()
    _bind(it, pts, 3)
    whole = _three_rounds(it, _third(N))
    _bind(it, pts[:45], 3)
    head = _three_rounds(it, _third(N)[:45])
    _bind(it, pts[45:], 3, seed_base=BOX["seed_base"] + 45, walk_seed_base=BOX["walk_seed_base"] + 45 * S)
    tail = _three_rounds(it, _third(N)[45:])
    it.close()
    assert np.any(whole["batches"] == 3) and np.any(whole["batches"] == 2)
    assert _same(whole, {k: np.concatenate([head[k], tail[k]]) for k in KEYS})

    listed = np.random.default_rng(6).uniform(0.1, 0.9, size=(50, 2)).astype(np.float32)
    other = np.random.default_rng(5).uniform(0.1, 0.9, size=(40, 2)).astype(np.float32)

    def run(with_list):
        """the frame solve, the carried frame solve, the carried point list and a single gradient call, with the rounds of the
        gradient list between them or without"""
        it = _box_it()
        seen, state = [], None
        it.solve()
        seen.append(it.solution.copy())
        it.points_carry(listed, 9, 16)
        seen.append(it.points_more(2))
        if with_list:
            _bind(it, pts, 3)
            it.gradient_points_more()
        seen.append(it.solve_gradient_points(other, 500, 1000, 32)["grad"])
        seen.append(it.points_more(3))
        if with_list:
            it.gradient_points_more(_third(N))
        it.solve_more(2)
        seen.append(it.solution.copy())
        if with_list:
            state = it.gradient_points_more()
        it.solve()
        seen.append(it.solution.copy())
        seen.append(it.points_more(1))
        assert it.points_done == 6 and it.spp_done == 2
        it.close()
        return seen, state

    plain, _ = run(False)
    mixed, state = run(True)
    assert _same(state, whole)
    assert np.any(plain[0] != 0) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(plain, mixed))


# ---- 3. restart, progress, the last round ----------------------------------------------------------------------------------------
def test_restart_repeats_the_bits_and_the_rounds_end_at_max_rounds():
    from elaina_amd.capi import WostError
    pts = _box_points()[:N]
    it = _box_it()
    _bind(it, pts, 2)
    it.gradient_points_more()
    first = it.gradient_points_more(_third(N))
    assert it.gradient_points_done == (N, 2)
    with pytest.raises(WostError, match="max_rounds"):
        it.gradient_points_more()
    assert it.gradient_points_done == (N, 2) and _same(it.gradient_points_carried(), first)
    it.gradient_points_restart()
    assert it.gradient_points_done == (N, 0)
    fresh = it.gradient_points_carried()
    assert np.all(fresh["batches"] == 0) and np.all(np.isnan(fresh["grad"])) and np.array_equal(fresh["radius"], first["radius"], equal_nan=True)
    it.gradient_points_more()
    assert _same(it.gradient_points_more(_third(N)), first)
    # a new bind replaces the list, an empty one releases it
    _bind(it, pts[:10], 1)
    assert it.gradient_points_done == (10, 0)
    _bind(it, pts[:0], 1)
    assert it.gradient_points_done == (0, 0)
    it.close()


# ---- 4. adaptive is the loop -------------------------------------------------------------------------------------------------------
def _converged(state, min_batches, abs_tol, rel_tol):
    """the documented test, in fp32 on the rounded outputs"""
    with np.errstate(invalid="ignore"):
        tol = np.maximum(np.float32(abs_tol), np.float32(rel_tol) * np.abs(state["grad"]))
        return (state["batches"] >= min_batches) & np.all(state["stderr"] <= tol, axis=(1, 2))


def _manual_loop(it, state, walkable, min_batches, max_batches, abs_tol, rel_tol, max_rounds):
    walks = 0
    while True:
        sel = walkable & ~_converged(state, min_batches, abs_tol, rel_tol) & (state["batches"] + 1 <= max_batches)
        if not sel.any() or it.gradient_points_done[1] >= max_rounds:
            return state, walks
        state = it.gradient_points_more(sel)
        walks += it.last_stats["walks_started"]


def _adaptive_is_the_loop(it, pts, batch_walks, eps, stride):
    n = len(pts)
    _bind(it, pts, 24, stride=stride, batch_walks=batch_walks)
    state = it.gradient_points_carried()
    walkable = _walkable(state, eps)
    for _ in range(3):
        state = it.gradient_points_more()
    # a tolerance between the points' errors after three rounds: some are below it at once, and a point more than twice above
    # it is still above at twelve batches (the error of K batches falls like 1 / sqrt(K))
    t = 0.7 * float(np.median(state["stderr"][walkable].max(axis=(1, 2))))
    assert np.isfinite(t) and t > 0.0
    it.gradient_points_restart()
    manual, walks = _manual_loop(it, it.gradient_points_carried(), walkable, 3, 12, t, 0.05, 24)
    K = manual["batches"]
    done = _converged(manual, 3, t, 0.05)
    early, late = walkable & (K < 12), walkable & (K == 12)
    assert early.any() and late.any(), (int(early.sum()), int(late.sum()))
    assert np.all(done[early]) and np.all(K[walkable] >= 3) and np.all(K[~walkable] == 0)
    it.gradient_points_restart()
    adaptive = it.gradient_points_adaptive(12, abs_tol=t, rel_tol=0.05, min_batches=3)
    assert _same(adaptive, manual) and it.last_stats["walks_started"] == walks == batch_walks * int(K.sum())
    assert it.gradient_points_done == (n, int(K.max()))
    # tighter: the call resumes, and no point loses a batch
    again = it.gradient_points_adaptive(20, abs_tol=t / 2, rel_tol=0.05, min_batches=3)
    K2 = again["batches"]
    assert np.all(K2 >= K) and np.any(K2 > K) and K2.max() <= 20
    assert it.last_stats["walks_started"] == batch_walks * int((K2 - K).sum())
    stopped = _converged(again, 3, t / 2, 0.05) | (K2 == 20)
    assert np.all(stopped[walkable]) or it.gradient_points_done[1] == 24
    # fewer rounds than the loop needs: it ends OK at the last round
    _bind(it, pts, 5, stride=stride, batch_walks=batch_walks)
    short = it.gradient_points_adaptive(12, abs_tol=t, rel_tol=0.05, min_batches=3)
    assert it.gradient_points_done == (n, 5) and short["batches"].max() == 5
    return t


def test_adaptive_is_the_manual_loop():
    it = _box_it()
    _adaptive_is_the_loop(it, _box_points()[:N], S, BOX["eps"], STRIDE)
    it.close()


# ---- 5. the device forms -----------------------------------------------------------------------------------------------------------
def test_device_forms_give_the_bits_of_the_host_forms():
    import torch
    pts = _box_points()[:N]
    it = _box_it()
    _bind(it, pts, 12)
    it.gradient_points_more()
    two = it.gradient_points_more()
    it.gradient_points_more(_third(N))
    t = 0.7 * float(np.nanmedian(two["stderr"].max(axis=(1, 2))))
    host = it.gradient_points_adaptive(8, abs_tol=t, rel_tol=0.05, min_batches=3)
    host_walks = it.last_stats["walks_started"]
    assert host_walks > 0

    stream = torch.cuda.current_stream().cuda_stream
    shapes = {"grad": (N, 2, 3), "stderr": (N, 2, 3), "field": (N, 3), "radius": (N,)}

    def arrays():
        d = {k: torch.full(shape, -1.0, dtype=torch.float32, device="cuda") for k, shape in shapes.items()}
        d["batches"] = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        return d

    def ptrs(d):
        return dict(stderr_ptr=d["stderr"].data_ptr(), field_ptr=d["field"].data_ptr(), radius_ptr=d["radius"].data_ptr(),
                    batches_ptr=d["batches"].data_ptr())

    def carry_dev(p):
        d_pts = torch.from_numpy(p).cuda()
        it.gradient_points_carry_dev(d_pts.data_ptr(), N, S, stream, STRIDE, 12, BOX["seed_base"], BOX["walk_seed_base"], BOX["seed_width"])

    carry_dev(pts)
    d = arrays()
    it.gradient_points_more_dev(d["grad"].data_ptr(), None, stream, **ptrs(d))
    it.gradient_points_more_dev(d["grad"].data_ptr(), None, stream, **ptrs(d))
    assert _same({k: v.cpu().numpy() for k, v in d.items()}, two)
    sel = torch.from_numpy(_third(N)).cuda()
    it.gradient_points_more_dev(d["grad"].data_ptr(), sel.data_ptr(), stream, **ptrs(d))
    stats = it.gradient_points_adaptive_dev(8, d["grad"].data_ptr(), stream, abs_tol=t, rel_tol=0.05, min_batches=3, **ptrs(d))
    assert _same({k: v.cpu().numpy() for k, v in d.items()}, host) and stats["walks_started"] == host_walks
    # only grad is required
    grad = torch.full((N, 2, 3), -1.0, dtype=torch.float32, device="cuda")
    it.gradient_points_more_dev(grad.data_ptr(), torch.zeros(N, dtype=torch.uint8, device="cuda").data_ptr(), stream)
    assert np.array_equal(grad.cpu().numpy(), host["grad"], equal_nan=True)
    # a NaN coordinate is never walked and answers NaN; its neighbours keep their bits
    bad = pts.copy()
    bad[37, 1] = np.nan
    carry_dev(bad)
    d = arrays()
    it.gradient_points_more_dev(d["grad"].data_ptr(), None, stream, **ptrs(d))
    stats = it.gradient_points_more_dev(d["grad"].data_ptr(), None, stream, **ptrs(d))
    dev = {k: v.cpu().numpy() for k, v in d.items()}
    assert all(np.all(np.isnan(dev[k][37])) for k in ("grad", "stderr", "field", "radius")) and dev["batches"][37] == 0
    rest = np.arange(N) != 37
    assert all(np.array_equal(dev[k][rest], two[k][rest], equal_nan=True) for k in KEYS)
    assert stats["walks_started"] == S * int((two["batches"][rest] > 0).sum())
    it.close()


# ---- 6. 3-D ----------------------------------------------------------------------------------------------------------------------------
def test_3d_batches_are_rows_and_adaptive_is_the_loop():
    """100 points in blocks of 32, 32, 32 and 4"""
    sd = _mixed_cube()
    pts = np.random.default_rng(7).uniform(0.05, 0.95, size=(100, 3)).astype(np.float32)
    sparse = np.zeros(100, np.uint8)
    sparse[40:50] = 1                        # block 1 alone
    sparse[97] = 1                           # ... and the partial block
    masks = [None, sparse, None]
    ref = _it3(sd, 16, 16, S, BOX["depth"], BOX["eps"])
    rows = _rows(ref, pts, 3, stride=100)
    ref.close()
    walkable = _walkable(rows[0], BOX["eps"])
    assert walkable.all()
    it = _it3(sd, 16, 16, S, BOX["depth"], BOX["eps"])
    _bind(it, pts, 3, stride=100)
    for r, m in enumerate(masks):
        out = it.gradient_points_more(m)
        assert out["grad"].shape == (100, 3, 3)
        _assert_state(out, _combine(rows[:r + 1], masks[:r + 1], walkable))
        assert it.last_stats["walks_started"] == S * (100 if m is None else int(m.sum()))
    _adaptive_is_the_loop(it, pts, S, BOX["eps"], 100)
    it.close()


# ---- 7. refusals that need the handle --------------------------------------------------------------------------------------------
def _refused(it, code, word, call):
    from elaina_amd.capi import WostError
    with pytest.raises(WostError, match=r"\(%d\).*%s" % (code, word)):
        call()


@pytest.mark.parametrize("dim", [2, 3])
def test_refusals_that_need_the_handle(dim):
    if dim == 2:
        make = lambda scene: _integrator(scene, 8, 8, 4, 8, 1e-3)
        plain, source = _mixed_box(), _with_source(_mixed_box(), 0.0, 1.0)
    else:
        make = lambda scene: _it3(scene, 8, 8, 4, 8, 1e-3)
        plain, source = _mixed_cube(), _mixed_cube()
        source["source"] = {"rgb": np.full((2, 2, 2, 3), 6.0, np.float32), "index_scale": (1.0, 1.0, 1.0), "index_offset": (0.0, 0.0, 0.0),
                            "intensity": 1.0}
    pts = np.full((6, dim), 0.5, np.float32)
    it = make(plain)
    for call in (it.gradient_points_more, it.gradient_points_carried, it.gradient_points_restart,
                 lambda: it.gradient_points_adaptive(8, abs_tol=0.1)):
        _refused(it, WOST_ERR_INVALID, "no gradient list is bound", call)
    _refused(it, WOST_ERR_INVALID, "n_pixels", lambda: it.gradient_points_carry(pts, 65, 6, 2, 0, 100, 16))      # S > 8 x 8
    assert it.gradient_points_done == (0, 0)
    it.gradient_points_carry(pts, 64, 6, 2, 0, 100, 16)                                                          # S = 8 x 8 fits
    it.gradient_points_more()
    # a refused bind leaves the list as it was
    _refused(it, WOST_ERR_INVALID, "n_pixels", lambda: it.gradient_points_carry(pts[:3], 65, 6, 2, 0, 100, 16))
    assert it.gradient_points_done == (6, 1)
    it.close()
    it = make(source)
    _refused(it, WOST_ERR_UNSUPPORTED, "source", lambda: it.gradient_points_carry(pts, 8, 6, 2, 0, 100, 16))
    it.close()


# ---- 8. sign and scale -------------------------------------------------------------------------------------------------------------
ANCHOR = dict(case="2d-mixed", S=64, rounds=16, seed_base=5, stride=64, walk_seed_base=4096, seed_width=64, k=4)


def test_the_carried_gradient_of_linear_boundary_data():
    """u = 1 + 2 y on the box with two Neumann sides: grad u = (0, 2) at every point.  After 16 full rounds of 64 walks every
    entry lies within k of its own batch-means standard error (15 degrees of freedom).  k: the single call's rows at these very
    seeds -- seed_base 5, round_stride 64, walk_seed_base 4096, seed_width 64 -- combined in numpy, which by test 1 is what the
    list computes, gave a largest ratio |grad - analytic| / grad_stderr of 3.1833 (rms of the errors over rms of the standard
    errors: 1.078); the next integer above it is 4, below the 6 that 15 degrees of freedom allow."""
    dim, scene, truth = ANALYTIC[ANCHOR["case"]]
    pts = np.random.default_rng(3).uniform(0.08, 0.92, size=(64, 2)).astype(np.float32)
    it = _integrator(scene(), LIN["frame"], LIN["frame"], 1, LIN["depth"], LIN["eps"])
    it.gradient_points_carry(pts, ANCHOR["S"], ANCHOR["stride"], ANCHOR["rounds"], ANCHOR["seed_base"], ANCHOR["walk_seed_base"], ANCHOR["seed_width"])
    for _ in range(ANCHOR["rounds"]):
        out = it.gradient_points_more()
    it.close()
    walkable = _walkable(out, LIN["eps"])
    assert walkable.all() and np.all(out["batches"] == ANCHOR["rounds"])
    err = np.abs(out["grad"].astype(np.float64) - np.asarray(truth, np.float64)[None, :, None])
    se = out["stderr"].astype(np.float64)
    print("largest |grad - analytic| / grad_stderr: %.3f" % float((err / se).max()))
    assert np.all(err <= ANCHOR["k"] * se), float((err / se).max())
