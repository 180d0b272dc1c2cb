"""The walk orders of a persistent launch (csrc/wost_order.h: order_by_distance, order_by_estimate) against a plain reference.

No field changes when these orders are wrong -- a pixel's arithmetic does not depend on the lane that runs it or on when --
so the parity tests cannot see them; only the solve's duration would move.  Here the product's own key kernels and sort run
on keys the test chose (tests/probe/wost_order_probe.hip, linked with a second compile of csrc/wost_order.hip) and the order
that comes back must equal, element for element, a reference written from the sentences of wost_order.h:

  distance   the bucket of a value is |d| with all but the top two mantissa bits cleared, as a bit pattern (so a NaN sits
             above +inf, by its pattern); descending by bucket, stable
  estimate   q = min(floor(max(e, 0) / 8), 4095); e >= 32760 gives 4095, a NaN gives 0; descending by q, stable

The CPU part checks the reference itself: against an O(n^2) selection that shares no code with it, and the prefix property
hand_over relies on -- for every T that is a multiple of 8 in [8, 32760] the first count(est >= T) entries are exactly those
walkers -- with the counter-example that shows why the bound is there."""
import math

import numpy as np
import pytest

import device_probe as dp
from device_probe import HIP_ERROR_INVALID_VALUE, HIP_SUCCESS, ORDER_SENTINEL, f32_from_bits

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 100003, 1048576)
BIG = 1048576                  # the walkers of config 2's frame
ORDER_MAX_THRESHOLD = 32760    # where the 12-bit estimate key saturates (wost_order.h)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def distance_bucket(d):
    bits = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32).astype(np.int64)
    magnitude = bits % (1 << 31)                       # the sign is dropped
    return magnitude - magnitude % (1 << 21)           # 23 mantissa bits, the top two stay


def estimate_key(e):
    e = np.asarray(e, dtype=np.float32).astype(np.float64)
    e = np.where(np.isnan(e), 0.0, e)
    return np.minimum(np.floor(np.maximum(e, 0.0) / 8.0), 4095.0).astype(np.int64)


def descending_stable(keys):
    return np.argsort(-np.asarray(keys, dtype=np.int64), kind="stable").astype(np.uint32)


def ref_by_distance(d):
    return descending_stable(distance_bucket(d))


def ref_by_estimate(e):
    return descending_stable(estimate_key(e))


REFERENCE = {"distance": ref_by_distance, "estimate": ref_by_estimate}


def prefix_property_holds(est, order, threshold):
    """the first count(est >= T) entries of the order are exactly the walkers with est >= T (a NaN is not >= T)"""
    est = np.asarray(est, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        is_long = est >= np.float32(threshold)
    count = int(is_long.sum())
    return set(np.asarray(order[:count]).tolist()) == set(np.flatnonzero(is_long).tolist())


# ---- a second derivation for small n: Python integers, selection instead of a sort ----------------------------------------------
def _py_distance_key(bits):
    bits &= 0x7FFFFFFF
    exponent, mantissa = bits >> 23, bits & 0x7FFFFF
    return exponent * 4 + mantissa // (1 << 21)


def _py_estimate_key(x):
    if math.isnan(x) or x <= 0.0:
        return 0
    if x >= 32760.0:
        return 4095
    return min(math.floor(x / 8.0), 4095)


def _py_keys(which, x):
    """a Python integer per value: the distance key from the value's bits (a float32 NaN does not survive the way through a
    Python float with its pattern), the estimate key from its value"""
    if which == "distance":
        return [_py_distance_key(b) for b in np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).tolist()]
    return [_py_estimate_key(float(v)) for v in x]


def selection_order(keys):
    """descending and stable, O(n^2): again and again the largest key left, the lowest index among equals"""
    left, out = list(range(len(keys))), []
    while left:
        best = left[0]
        for i in left[1:]:
            if keys[i] > keys[best]:
                best = i
        out.append(best)
        left.remove(best)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def distance_edges():
    bits = []
    for exponent in (1, 64, 127, 128, 200, 254):
        for mantissa in (0x1FFFFF, 0x200000, 0x3FFFFF, 0x400000, 0x7FFFFF):
            b = (exponent << 23) | mantissa
            bits += [b - 1, b, b + 1]                                   # (0x7FFFFF + 1 carries into the exponent: 254 -> +inf)
    specials = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x7F7FFFFF, 0x7F800000,
                0x7FC00000, 0x7F800001, 0x7FA00000, 0x7FFFFFFF, 0xFFC00000,               # NaNs of several buckets, one negative
                0xBF800000, 0xC0600000, 0xFF7FFFFF, 0xFF800000, 0x80000001]               # -1, -3.5, -FLT_MAX, -inf, -tiny
    negatives = [b | 0x80000000 for b in bits[::4]]
    return f32_from_bits(bits + specials + negatives)


ESTIMATE_EDGES = np.asarray([-1.0, -0.0, 0.0, np.nan, np.inf, 7.9999995, 8.0, 15.999999, 16.0, 32751.998, 32752.0, 32759.998, 32760.0,
                             32768.0, 65528.0, 1e9], np.float32)
ESTIMATE_EDGES = np.concatenate([ESTIMATE_EDGES, dp.F32_TINY.reshape(1)])


def _fill(edges, n, filler, rng):
    """n values: the edges (a seeded choice of them where n is smaller), the rest from filler(count), all shuffled"""
    if n <= len(edges):
        x = rng.permutation(edges)[:n]
    else:
        x = np.concatenate([edges, filler(n - len(edges)).astype(np.float32)])
    return rng.permutation(x).astype(np.float32)


def make_input(which, kind, n):
    rng = np.random.default_rng([n, sum(map(ord, which + kind))])
    i = np.arange(n, dtype=np.int64)
    if which == "distance":
        if kind == "equal":
            return np.full(n, 3.5, np.float32)
        if kind in ("ascending", "descending"):
            x = f32_from_bits(0x30000000 + i * 512)                       # strictly ascending, 2^-31 ... 2^33 at the largest n
            return np.ascontiguousarray(x if kind == "ascending" else x[::-1])
        if kind == "loguniform":
            return rng.permutation((10.0 ** rng.uniform(-12.0, 12.0, n)).astype(np.float32))
        if kind == "runs":                                                # two buckets in runs of 37
            return np.where((i // 37) % 2 == 0, 1.0, 1.5).astype(np.float32)
        if kind == "one_bucket_runs":                                     # two values of one bucket: nothing moves
            return np.where((i // 37) % 2 == 0, 1.0, 1.2).astype(np.float32)
        if kind == "mixed":
            return _fill(distance_edges(), n, lambda k: 10.0 ** rng.uniform(-12.0, 12.0, k), rng)
    else:
        if kind == "zeros":
            return np.zeros(n, np.float32)
        if kind == "all_long":
            x = rng.uniform(32760.0, 70000.0, n).astype(np.float32)
            x[::5] = 32760.0
            x[3::11] = np.inf
            return x
        if kind == "mixed":
            def filler(k):
                ints = rng.integers(0, 70000, k).astype(np.float64)
                return np.where(rng.random(k) < 0.5, ints, rng.uniform(0.0, 70000.0, k))
            return _fill(ESTIMATE_EDGES, n, filler, rng)
    raise KeyError((which, kind))


KINDS = {"distance": ("equal", "ascending", "descending", "loguniform", "runs", "one_bucket_runs", "mixed"),
         "estimate": ("mixed", "all_long", "zeros")}
IDENTITY_KINDS = {("distance", "equal"), ("distance", "descending"), ("distance", "one_bucket_runs"), ("estimate", "zeros"),
                  ("estimate", "all_long")}
_CASES = {}


def case(which, kind, n):
    """(input, reference order), read-only; the mixed inputs serve several tests and are made once"""
    if (which, kind, n) in _CASES:
        return _CASES[which, kind, n]
    x = make_input(which, kind, n)
    want = REFERENCE[which](x)
    x.setflags(write=False)
    want.setflags(write=False)
    if kind == "mixed":
        _CASES[which, kind, n] = (x, want)
    return x, want


# ---- CPU: the reference is what the sentences say -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 65, 255, 300])
def test_reference_equals_a_selection_without_a_sort(n):
    for which in ("distance", "estimate"):
        for kind in KINDS[which]:
            x, want = case(which, kind, n)
            assert selection_order(_py_keys(which, x)) == want.tolist(), (which, kind)
            if (which, kind) in IDENTITY_KINDS:
                assert want.tolist() == list(range(n)), (which, kind)


def test_reference_on_every_edge_value():
    """all the edges at once (the sized inputs above hold a choice of them where n is small)"""
    for which, edges in (("distance", distance_edges()), ("estimate", ESTIMATE_EDGES)):
        x = np.random.default_rng(7).permutation(edges)
        assert len(x) <= 300
        assert selection_order(_py_keys(which, x)) == REFERENCE[which](x).tolist()
    # what the sentences say about single values
    b = distance_bucket(f32_from_bits([0x3F800000, 0x3F9FFFFF, 0x3FA00000, 0xBF800000, 0x7F800000, 0x7F800001, 0x7FA00000, 0x00000001, 0x0]))
    assert b[0] == b[1] == b[3] and b[2] > b[1] and b[5] == b[4] and b[6] > b[4] and b[7] == b[8] == 0
    q = estimate_key(np.asarray([-1.0, np.nan, 7.9999995, 8.0, 32759.998, 32760.0, 65528.0, np.inf], np.float32))
    assert q.tolist() == [0, 0, 0, 1, 4094, 4095, 4095, 4095]


def _estimate_property_inputs():
    t = np.arange(8, 32768 + 8, 8).astype(np.float32)
    around_every_threshold = np.random.default_rng(11).permutation(np.concatenate([t, np.nextafter(t, np.float32(0.0)), ESTIMATE_EDGES]))
    return [around_every_threshold, case("estimate", "mixed", 300)[0], case("estimate", "mixed", 4097)[0], case("estimate", "all_long", 300)[0],
            case("estimate", "zeros", 64)[0], np.random.default_rng(12).permutation(ESTIMATE_EDGES)]


def test_prefix_property_of_the_estimate_order_up_to_its_bound():
    """what hand_over relies on (ord / ord + n_long): for every T that is a multiple of 8 in [8, 32760]"""
    for est in _estimate_property_inputs():
        order = ref_by_estimate(est)
        with np.errstate(invalid="ignore"):
            sorted_est = est[order]
            for threshold in range(8, ORDER_MAX_THRESHOLD + 8, 8):
                is_long = sorted_est >= np.float32(threshold)
                count = int(is_long.sum())
                assert is_long[:count].all(), threshold          # (a permutation: the same as the equality of the two sets)
        for threshold in (8, 1024, 32752, ORDER_MAX_THRESHOLD):
            assert prefix_property_holds(est, order, threshold)


def test_prefix_property_fails_beyond_the_bound():
    """why long_steps stops at 32760: every estimate from there on has the key 4095, so the stable order keeps them in input
    order and the first count(est >= 32768) entries hold 32760 in place of 65528"""
    est = np.asarray([32760.0, 40000.0, 32767.0, 65528.0], np.float32)
    order = ref_by_estimate(est)
    assert order.tolist() == [0, 1, 2, 3]
    assert prefix_property_holds(est, order, ORDER_MAX_THRESHOLD)
    assert not prefix_property_holds(est, order, 32768)


# ---- GPU: the product's orders equal the reference ---------------------------------------------------------------------------
def _assert_run(probe, which, x, want, what):
    n = len(x)
    rc, out, other = probe.run(probe.BY_DISTANCE if which == "distance" else probe.BY_ESTIMATE, x)
    assert rc == HIP_SUCCESS, (what, rc)
    got = out[:n]
    if not np.array_equal(got, want):
        k = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: first difference at position %d of %d: slot %d (key %r) for slot %d (key %r)" % (
            what, k, n, got[k], x[got[k]] if got[k] < n else None, want[k], x[want[k]]))
    assert (out[n:] == ORDER_SENTINEL).all(), what + ": an entry behind the n-th was written"
    assert (other[n:] == ORDER_SENTINEL).all(), what + ": an entry behind the n-th of the first value buffer was written"


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_orders_equal_the_reference(n):
    """cap == n: a WalkOrder sized for exactly these walkers"""
    with dp.WalkOrderProbe(n) as probe:
        for which in ("distance", "estimate"):
            for kind in KINDS[which]:
                x, want = case(which, kind, n)
                if (which, kind) in IDENTITY_KINDS:
                    assert np.array_equal(want, np.arange(n, dtype=np.uint32))
                _assert_run(probe, which, x, want, "%s/%s n=%d" % (which, kind, n))


@pytest.mark.gpu
def test_one_scratch_serves_runs_of_every_size():
    """as in the product: the scratch is sized once for the frame and reused with fewer walkers.  Largest first, smallest last,
    then the largest again: no key of a longer run may leak into a shorter one, and the entries behind the n-th stay untouched"""
    sizes = sorted(SIZES, reverse=True) + [BIG]
    with dp.WalkOrderProbe(BIG) as probe:
        for n in sizes:
            for which in ("distance", "estimate"):
                x, want = case(which, "mixed", n)
                _assert_run(probe, which, x, want, "%s n=%d of cap %d" % (which, n, BIG))


@pytest.fixture(scope="module")
def largest_long_steps():
    """the largest value wost_set_option("long_steps") accepts, asked of the library itself"""
    from conftest import box_problem
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings
    from elaina_amd.capi import WostError
    it = UniformIntegrator(box_problem(), UniformIntegratorSettings((8, 8), 1, 4, 1e-3))
    accepted = []
    for value in range(0, 131072 + 8, 8):
        try:
            it.set_option("long_steps", value)
            accepted.append(value)
        except WostError:
            pass
    it.close()
    assert accepted and accepted[0] == 0
    return max(accepted)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4097, 100003])
def test_the_prefix_contract_of_hand_over(largest_long_steps, n):
    """hand_over sends order[:count_long] beside the rounds and gives the first round order[count_long:], where count_long is
    the walk kernel's count of est >= long_steps: for every threshold the option accepts, the largest included, the prefix is
    exactly those walkers and the rest is in stable descending order"""
    thresholds = [8, 16, 1024, 32752, 32760, largest_long_steps]
    t = np.asarray(sorted(set(thresholds)), np.float32)
    base, _ = case("estimate", "mixed", n)
    around = np.concatenate([t, np.nextafter(t, np.float32(0.0)), np.nextafter(t, np.float32(np.inf)), t - 8, t + 8])
    est = np.random.default_rng(n).permutation(np.concatenate([base[:n - 4 * len(around)], np.tile(around, 4)])).astype(np.float32)
    assert len(est) == n
    with dp.WalkOrderProbe(n) as probe:
        rc, order, _ = probe.by_estimate(est)
    assert rc == HIP_SUCCESS
    q = estimate_key(est)
    for threshold in thresholds:
        with np.errstate(invalid="ignore"):
            is_long = est >= np.float32(threshold)
        count = int(is_long.sum())
        assert 0 < count < n
        assert set(order[:count].tolist()) == set(np.flatnonzero(is_long).tolist()), threshold
        rest = np.flatnonzero(~is_long)
        assert np.array_equal(order[count:], rest[np.argsort(-q[rest], kind="stable")]), threshold


@pytest.mark.gpu
def test_no_walkers_is_a_success_that_writes_nothing():
    with dp.WalkOrderProbe(64) as probe:
        for which in (probe.BY_DISTANCE, probe.BY_ESTIMATE):
            rc, out, other = probe.run(which, np.zeros(0, np.float32))
            assert rc == HIP_SUCCESS
            assert (out == ORDER_SENTINEL).all() and (other == ORDER_SENTINEL).all()


@pytest.mark.gpu
def test_more_walkers_than_the_scratch_holds_are_refused():
    with dp.WalkOrderProbe(64) as probe:
        for which in (probe.BY_DISTANCE, probe.BY_ESTIMATE):
            rc, out, other = probe.run(which, np.arange(65, dtype=np.float32))
            assert rc == HIP_ERROR_INVALID_VALUE
            assert (out == ORDER_SENTINEL).all() and (other == ORDER_SENTINEL).all()
        # (and the handle still serves a run that fits)
        x, want = case("estimate", "mixed", 64)
        _assert_run(probe, "estimate", x, want, "after a refusal")
