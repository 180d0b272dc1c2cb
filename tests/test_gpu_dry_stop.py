"""The persistent launch's global look at the dry queue (wost_set_option "dry_stop", "dry_cadence"): once no input slot is
unread every wave stops at its next look at the cursor, not only a wave that needs a refill.  Which launch walks which step
of a pixel never mattered to the bits, so both rules must give the oracle's field and counters bit for bit; and at config 2's
size the rule must be seen to act: more walkers handed over than the wave-local rule can hand over at all."""
import numpy as np
import pytest

from test_gpu_parity import _assert_same_solve, _cached_ref, _with_source

pytestmark = pytest.mark.gpu

DRY = [0, 1]


@pytest.mark.parametrize("dry_stop", DRY)
@pytest.mark.parametrize("opts", [
    {"resident_blocks": 2, "dry_cadence": 1}, {"resident_blocks": 2}, {"resident_blocks": 6, "dry_cadence": 1}, {"resident_blocks": 6},
    {"resident_blocks": 2, "dry_cadence": 1, "block_size": 64}, {"resident_blocks": 2, "block_size": 64},
    {"resident_blocks": 6, "dry_cadence": 1, "block_size": 64}, {"resident_blocks": 6, "block_size": 64},
], ids=lambda o: "-".join("%s%d" % (k[:5], v) for k, v in o.items()))
def test_ladybug_same_bits_under_both_rules(oracle, ladybug, opts, dry_stop):
    """several waves, several pixels per lane: 7 680 pixels on 512 or 1 536 lanes (128 or 384 with blocks of one wave)"""
    ref = _cached_ref(oracle, ladybug, "persist-ladybug", 96, 80, 24, 64, 1.0)
    _assert_same_solve(oracle, ladybug, 96, 80, 24, 64, 1.0, ref=ref, persist=1, dry_stop=dry_stop, **opts)


@pytest.mark.parametrize("dry_stop", DRY)
def test_fille_same_bits_under_both_rules(oracle, fille, dry_stop):
    ref = _cached_ref(oracle, fille, "persist-fille", 96, 80, 9, 128, 1.0)
    _assert_same_solve(oracle, fille, 96, 80, 9, 128, 1.0, ref=ref, persist=1, dry_stop=dry_stop, resident_blocks=8, long_steps=16)


@pytest.mark.parametrize("dry_stop", DRY)
def test_masked_mixed_boundary_box_same_bits_under_both_rules(oracle, dry_stop):
    from conftest import box_problem
    p = box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.3 * (s - 2))
    p.mask = (np.arange(70 * 50) % 3 != 0).astype(np.uint8)
    ref = _cached_ref(oracle, p, "dry-masked-box", 70, 50, 12, 32, 1e-3)
    _assert_same_solve(oracle, p, 70, 50, 12, 32, 1e-3, ref=ref, persist=1, dry_stop=dry_stop, resident_blocks=2)
    assert np.all(ref["field"][p.mask == 0] == 0)


@pytest.mark.parametrize("dry_stop", DRY)
def test_open_polyline_from_afar_same_bits_under_both_rules(oracle, dry_stop):
    """most walks stray beyond the plain visits' range: a lane whose walker strays goes for a refill while other waves stop
    on the global look"""
    from elaina_amd import Problem
    t = np.linspace(0.0, 1.0, 301)
    verts = np.stack([100.0 * t, 20.0 * np.sin(9.0 * t) + 5.0 * np.cos(31.0 * t)], 1).astype(np.float32)
    segs = np.stack([np.arange(300), np.arange(300) + 1], 1).astype(np.int32)
    cols = np.random.default_rng(5).uniform(0.0, 1.0, size=(301, 6)).astype(np.float32)
    q = Problem(d_verts=verts, d_segs=segs, d_colors=cols, probe=(300.0, 50.0, 0.0, 0.0, 1.0))
    ref = _cached_ref(oracle, q, "dry-polyline", 64, 64, 6, 12, 0.5)
    _assert_same_solve(oracle, q, 64, 64, 6, 12, 0.5, ref=ref, persist=1, dry_stop=dry_stop, resident_blocks=2)


@pytest.mark.parametrize("dry_stop", DRY)
def test_source_term_same_bits_under_both_rules(oracle, dry_stop):
    from conftest import box_problem
    mixed = _with_source(box_problem(d_sides=(0, 2), n_sides=(1, 3), value=lambda x, y: y, flux=lambda x, y, s: 0.2), 0.0, 1.0)
    ref = _cached_ref(oracle, mixed, "dry-source-box", 48, 40, 14, 32, 1e-3)
    _assert_same_solve(oracle, mixed, 48, 40, 14, 32, 1e-3, ref=ref, persist=1, dry_stop=dry_stop, resident_blocks=2)


@pytest.fixture(scope="module")
def config2_solves(ladybug):
    """config 2 (1024^2, 256 spp) solved twice with the global look and once without: field, counters and launches of each"""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    it = UniformIntegrator(ladybug, UniformIntegratorSettings((1024, 1024), 256, 64, 1.0))
    out = []
    for dry_stop in (1, 1, 0):
        it.set_option("dry_stop", dry_stop)
        it.solve()
        out.append((it.solution.copy(), dict(it.last_stats), it.last_launches()))
    it.close()
    return out


def _handed_over_and_bound(launches):
    """the walkers the launch after the persistent one takes plus those that run beside it, and the most the wave-local rule
    can hand over: every resident lane but one per wave (a wave stops there when one of its lanes finds no unread slot)"""
    from elaina_amd import capi
    assert launches[0]["kind"] == capi.LAUNCH_PERSISTENT
    lanes = launches[0]["grid"] * 256
    return launches[1]["walkers"] + launches[1]["walkers_beside"], lanes - lanes // 64


def test_the_rule_acts_at_config2(config2_solves):
    (_, s1, l1), _, (_, s0, l0) = config2_solves
    assert s1["walk_steps"] == 1949024384 == s0["walk_steps"]
    got, bound = _handed_over_and_bound(l1)
    print("dry_stop 1: handed over", got, "wave-local bound", bound)
    assert got > bound
    got0, bound0 = _handed_over_and_bound(l0)
    print("dry_stop 0: handed over", got0, "wave-local bound", bound0)
    assert got0 <= bound0


def test_results_do_not_depend_on_which_wave_stops_when(config2_solves):
    (a, sa, _), (b, sb, _), (c, sc, _) = config2_solves
    assert np.array_equal(a, b)
    assert np.array_equal(a, c)
    for k in ("walk_steps", "walks_started", "walks_absorbed", "walks_truncated", "neumann_hits"):
        assert sa[k] == sb[k] == sc[k], k
