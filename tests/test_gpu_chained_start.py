"""The chained start of the round and quad kernels (wost_set_option "chain_start"): a lane whose walk is absorbed takes the
depth-0 step of its pixel's next sample -- the closest point of the evaluation point is cached -- in the same step trip, not
in the wave's next one.  The arithmetic of that step, the order of a pixel's samples and its random stream are what they
were, so both rules must give the oracle's field and its five counters bit for bit, in every kind of launch; and the rule must
be seen to act: the same walk steps in fewer trips of the scheduler loop."""
import numpy as np
import pytest

from conftest import box_problem, wiggly_problem
from test_gpu_parity import THREADS, _assert_same_solve, _cached_ref, _integrator, _with_source

pytestmark = pytest.mark.gpu

CHAIN = [0, 1]
COUNTERS = ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits")


def _ids(o):
    return "-".join("%s%d" % (k[:5], v) for k, v in o.items()) or "defaults"


# ---- the ladybug frame: persistent launch, rounds of every critical length, quads, the long remainders ------------------------
@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("opts", [
    {"persist": 1, "resident_blocks": 2}, {"persist": 1, "resident_blocks": 6},
    {"persist": 1, "resident_blocks": 2, "block_size": 64}, {"persist": 1, "resident_blocks": 6, "block_size": 64},
    # plain rounds: 1 step never chains, 2 spend the whole budget on one chain, 3 leave one step behind a chain
    {"steps_per_round": 1}, {"steps_per_round": 2}, {"steps_per_round": 3}, {"steps_per_round": 7}, {"steps_per_round": 256},
    # four lanes per walker in every round; short quad rounds on blocks of one wave
    {"quad": 1}, {"quad": 1, "steps_per_round": 2}, {"quad": 1, "steps_per_round": 7, "block_size": 64},
    # the launch of the long remainders beside the rounds
    {"persist": 1, "resident_blocks": 2, "long_steps": 16},
], ids=_ids)
def test_ladybug_same_bits_under_both_rules(oracle, ladybug, opts, chain):
    ref = _cached_ref(oracle, ladybug, "persist-ladybug", 96, 80, 24, 64, 1.0)
    _assert_same_solve(oracle, ladybug, 96, 80, 24, 64, 1.0, ref=ref, chain_start=chain, **opts)


@pytest.mark.parametrize("chain", CHAIN)
def test_fille_same_bits_under_both_rules(oracle, fille, chain):
    ref = _cached_ref(oracle, fille, "persist-fille", 96, 80, 9, 128, 1.0)
    _assert_same_solve(oracle, fille, 96, 80, 9, 128, 1.0, ref=ref, persist=1, chain_start=chain, resident_blocks=8, long_steps=16)


# ---- walks of one and two steps; one and two samples -------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 1}, {"quad": 1}], ids=_ids)
def test_depth_limits_one_and_two(oracle, ladybug, opts, depth, chain):
    """depth limit 1: the chained step is truncated at once and the walk that follows starts the ordinary way"""
    ref = _cached_ref(oracle, ladybug, "chain-depth%d" % depth, 48, 40, 6, depth, 1.0)
    assert ref["walks_truncated"] > 0
    _assert_same_solve(oracle, ladybug, 48, 40, 6, depth, 1.0, ref=ref, chain_start=chain, **opts)


@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 1}, {"quad": 1}], ids=_ids)
def test_one_and_two_samples(oracle, ladybug, opts, spp, chain):
    """nothing chains at one sample; a pixel's last sample never chains"""
    ref = _cached_ref(oracle, ladybug, "chain-spp%d" % spp, 48, 40, spp, 64, 1.0)
    _assert_same_solve(oracle, ladybug, 48, 40, spp, 64, 1.0, ref=ref, chain_start=chain, **opts)


# ---- evaluation points inside the shell: their depth-0 step absorbs again and stays on the old path -----------------------------
SHELL = dict(w=70, h=50, spp=8, depth=32, eps=0.2)


def _shell_box():
    return box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: 1.0 + x + 2.0 * y)


def _fraction_inside_shell():
    """the share of the frame's evaluation points within eps of the Dirichlet sides y = 0 and y = 1 of the unit box, in the
    arithmetic of eval_point (probe: scale 0.45 around (0.5, 0.5), up = +y)"""
    py = np.repeat(np.arange(SHELL["h"], dtype=np.float32), SHELL["w"])
    ndc = np.float32(2.0) * py / np.float32(SHELL["h"]) + np.float32(-1.0)
    y = np.float32(0.45) * ndc + np.float32(0.5)
    dist = np.minimum(y, np.float32(1.0) - y)
    return float(np.mean(dist < np.float32(SHELL["eps"])))


@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("opts", [{}, {"steps_per_round": 3, "block_size": 64}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}], ids=_ids)
def test_pixels_inside_the_shell(oracle, opts, chain):
    inside = _fraction_inside_shell()
    print("evaluation points inside the shell: %.1f %%" % (100.0 * inside))
    assert 0.05 < inside < 0.95       # both kinds of pixel are present
    p = _shell_box()
    s = SHELL
    ref = _cached_ref(oracle, p, "chain-shell-box", s["w"], s["h"], s["spp"], s["depth"], s["eps"])
    # a pixel inside the shell is absorbed at depth 0 in every sample: at least that many walks of one step
    assert ref["walks_absorbed"] >= int(inside * s["w"] * s["h"]) * s["spp"]
    _assert_same_solve(oracle, p, s["w"], s["h"], s["spp"], s["depth"], s["eps"], ref=ref, chain_start=chain, **opts)


# ---- flat emissive Neumann sides: the chained step makes the sampleNeumann draws ----------------------------------------------
def _emissive_box():
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.3 * (s - 2))
    p.mask = (np.arange(70 * 50) % 3 != 0).astype(np.uint8)
    return p


@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1, "steps_per_round": 3}], ids=_ids)
def test_masked_emissive_box(oracle, opts, chain):
    p = _emissive_box()
    ref = _cached_ref(oracle, p, "dry-masked-box", 70, 50, 12, 32, 1e-3)
    assert ref["neumann_hits"] > 0
    _assert_same_solve(oracle, p, 70, 50, 12, 32, 1e-3, ref=ref, chain_start=chain, **opts)
    assert np.all(ref["field"][p.mask == 0] == 0)


@pytest.mark.parametrize("chain", CHAIN)
def test_three_shards_of_the_emissive_box_sum_to_the_frame(oracle, chain):
    import torch
    p = _emissive_box()
    ref = _cached_ref(oracle, p, "dry-masked-box", 70, 50, 12, 32, 1e-3)
    it = _integrator(p, 70, 50, 12, 32, 1e-3)
    it.set_option("chain_start", chain)
    total = torch.zeros(70 * 50 * 3, dtype=torch.float32, device="cuda")
    sums = dict.fromkeys(COUNTERS, 0)
    for r in range(3):
        buf = torch.zeros(70 * 50 * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = it.solve_sharded(r, 3, buf.data_ptr())
        for c in COUNTERS:
            sums[c] += st[c]
        total += buf
    it.close()
    for c in COUNTERS:
        assert sums[c] == ref[c], c
    assert np.array_equal(total.cpu().numpy().reshape(-1, 3), ref["field"])


# ---- a source term: the chained step makes the sampleSource draws --------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("opts", [{"steps_per_round": 3, "block_size": 64}, {"persist": 1, "resident_blocks": 2}], ids=_ids)
def test_source_term(oracle, opts, chain):
    mixed = _with_source(box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.2), 0.0, 1.0)
    ref = _cached_ref(oracle, mixed, "dry-source-box", 48, 40, 14, 32, 1e-3)
    _assert_same_solve(oracle, mixed, 48, 40, 14, 32, 1e-3, ref=ref, chain_start=chain, **opts)


# ---- a Neumann mesh on the tree: the unchanged wave-cooperative steps beside the changed round and quad code -----------------------
@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("opts", [{}, {"coop": 0}, {"quad": 1}], ids=_ids)
def test_tree_borne_neumann_mesh(oracle, opts, chain):
    p = wiggly_problem(emissive=True)
    ref = _cached_ref(oracle, p, "chain-wiggly", 40, 40, 2, 24, 0.05)
    _assert_same_solve(oracle, p, 40, 40, 2, 24, 0.05, ref=ref, chain_start=chain, **opts)


# ---- continued solves: the carried generator state after a chained last-but-one sample --------------------------------------------
@pytest.mark.parametrize("chain", CHAIN)
@pytest.mark.parametrize("opts", [{}, {"persist": 1, "resident_blocks": 2}, {"quad": 1}], ids=_ids)
def test_continued_solve_in_three_cuts(oracle, fille, opts, chain):
    ref = _cached_ref(oracle, fille, "persist-fille", 96, 80, 9, 128, 1.0)
    it = _integrator(fille, 96, 80, 4, 128, 1.0)
    it.set_option("chain_start", chain)
    for k, v in opts.items():
        it.set_option(k, v)
    sums = dict.fromkeys(COUNTERS, 0)
    for more in (3, 5, 1):
        it.solve_more(more)
        for c in COUNTERS:
            sums[c] += it.last_stats[c]
    assert it.spp_done == 9
    for c in COUNTERS:
        assert sums[c] == ref[c], c
    assert np.array_equal(it.solution, ref["field"]), float(np.abs(it.solution - ref["field"]).max())
    it.close()


# ---- a point solve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAIN)
def test_solve_points_on_500_points(oracle, ladybug, chain):
    """the first 500 evaluation points of the 96-wide frame on the streams of its first 500 pixels: the oracle's solve of
    that range of pixels; a persistent launch of one wave, so the points pass through lanes, hand-over and quads"""
    from test_gpu_points import _grid_points
    key = "chain-points-500"
    from test_gpu_parity import _REF_CACHE
    if key not in _REF_CACHE:
        _REF_CACHE[key] = oracle.solve(ladybug.as_dict(), 96, 80, 24, 64, 1.0, pixel_begin=0, pixel_end=500, threads=THREADS)
    ref = _REF_CACHE[key]
    pts = _grid_points(oracle, ladybug, 96, 80)[:500]
    it = _integrator(ladybug, 96, 80, 24, 64, 1.0)
    it.set_option("chain_start", chain)
    it.set_option("persist", 1)
    it.set_option("resident_blocks", 1)
    it.set_option("block_size", 64)
    field = it.solve_points(pts, 0, 96)
    for c in COUNTERS:
        assert it.last_stats[c] == ref[c], c
    assert np.array_equal(field, ref["field"])
    it.close()


# ---- the rule acts -----------------------------------------------------------------------------------------------------------
def test_the_rule_acts(ladybug):
    """the same walk steps in strictly fewer step trips and traversal trips of the scheduler loop"""
    it = _integrator(ladybug, 96, 80, 24, 64, 1.0)
    it.set_option("persist", 1)
    it.set_option("resident_blocks", 6)
    got = {}
    for chain in CHAIN:
        it.set_option("chain_start", chain)
        it.solve()
        got[chain] = dict(it.last_stats)
        print("chain_start", chain, {k: got[chain][k] for k in ("walk_steps", "step_trips", "trav_trips")})
    it.close()
    print("step trips x %.4f, traversal trips x %.4f" % (got[1]["step_trips"] / got[0]["step_trips"],
                                                       got[1]["trav_trips"] / got[0]["trav_trips"]))
    assert got[1]["walk_steps"] == got[0]["walk_steps"] > 0
    assert got[1]["step_trips"] < got[0]["step_trips"]
    assert got[1]["trav_trips"] < got[0]["trav_trips"]


def test_option_takes_zero_and_one_only(ladybug):
    it = _integrator(ladybug, 8, 8, 1, 4, 1.0)
    for bad in (-1, 2, 0.5):
        with pytest.raises(Exception):
            it.set_option("chain_start", bad)
    it.set_option("chain_start", 0)
    it.set_option("chain_start", 1)
    it.close()
