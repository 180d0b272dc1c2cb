"""The deterministic math functions, function by function, at inputs chosen here (tests/device_probe.py).

(a) gpu: the device's inline functions (csrc/wost_math.h, wost_device3.h, wost_vmm_device.h, reached through the probe library
    tests/probe/wost_probe.hip that is built with the product library's flags) equal the oracle's (oracle/wost_detmath.h,
    wost_oracle.c, through oracle/wost_probe.c) bit for bit on the whole input set -- NaN equals NaN, the sign of zero counts.
(b) cpu: the oracle's functions against a high-precision reference -- numpy float64 of the exact float argument for the fp32
    functions, mpmath at 40 digits for the fp64 ones -- within the bounds DESIGN.md section 2.1 states; every test prints its
    worst error and where it occurred.
(c) cpu: the values at out-of-domain arguments, pinned on the oracle; (a) carries them to the device.
"""
import math
import os

import numpy as np
import pytest

import device_probe as dp
from oracle.oracle import PROBE_FUNCTIONS

_ORACLE_OUT = {}


def oracle_out(oracle, fn):
    """the oracle's results on the whole input set of fn: computed once, shared, read-only"""
    if fn not in _ORACLE_OUT:
        out = oracle.probe(fn, dp.input_set(fn))
        out.setflags(write=False)
        _ORACLE_OUT[fn] = out
    return _ORACLE_OUT[fn]


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- (a) device == oracle -------------------------------------------------------------------------------------------------
def _rows_that_differ(got, ref):
    """indices of the results that are not the same value: every NaN is one value, everything else, the sign of zero
    included, goes by its bits"""
    assert got.shape == ref.shape and got.dtype == ref.dtype
    gb, rb = _bits(got), _bits(ref)
    if got.dtype.kind == "f":
        gn, rn = np.isnan(got), np.isnan(ref)
        differ = np.where(gn | rn, gn != rn, gb != rb)
    else:
        differ = gb != rb
    return np.flatnonzero(differ.reshape(len(ref), -1).any(axis=1))


def test_probe_is_built_with_the_library_flags():
    """the probe tests what the product's flags make of the headers: both builds record the flag list they compiled with"""
    from elaina_amd import build as b
    assert os.path.exists(b.PROBE_PATH), "run `python __graft_entry__.py`"
    stamps = [open(os.path.join(b.OBJ_DIR, name)).read() for name in ("flags.stamp", "probe_flags.stamp")]
    assert stamps[0] == stamps[1]


def test_comparison_counts_nan_zero_sign_and_last_bit():
    f = np.float32
    ref = np.asarray([[1.0, np.nan], [0.0, 2.0], [np.nan, 3.0], [-0.0, 1.0], [5.0, 6.0]], f)
    same = ref.copy()
    same[0, 1] = dp.f32_from_bits(0xFFC00001)                  # another NaN
    assert len(_rows_that_differ(same, ref)) == 0
    other = ref.copy()
    other[1, 0] = -0.0                                          # sign of zero
    other[2, 0] = 7.0                                           # a number for a NaN
    other[4, 1] = np.nextafter(f(6.0), f(7.0))                  # last bit
    assert _rows_that_differ(other, ref).tolist() == [1, 2, 4]
    u = np.asarray([1, 2, 3], np.uint64)
    assert _rows_that_differ(u + np.asarray([0, 1, 0], np.uint64), u).tolist() == [1]


@pytest.mark.gpu
@pytest.mark.parametrize("fn", sorted(PROBE_FUNCTIONS, key=lambda k: PROBE_FUNCTIONS[k][0]))
def test_gpu_device_equals_oracle(oracle, fn):
    x = dp.input_set(fn)
    ref = oracle_out(oracle, fn)
    got = dp.device_probe(fn, x)
    bad = _rows_that_differ(got, ref)
    xs = x.reshape(len(ref), -1)
    print("%s: %d arguments, %d differ" % (fn, len(ref), len(bad)))
    assert len(bad) == 0, "%s: %d of %d differ, first at argument %r: device %r, oracle %r" % (
        fn, len(bad), len(ref), xs[bad[0]], got[bad[0]], ref[bad[0]])


# ---- (b) oracle vs high precision ------------------------------------------------------------------------------------------
def _ulp32(ref):
    """ulp of the fp32 binade that holds |ref| (ref: float64, normal range of fp32)"""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, e - 24)


def _report(name, err, x, unit):
    i = int(np.argmax(err))
    print("%s: worst error %.4g %s at argument %r (%s), %d arguments" % (name, err[i], unit, x[i], float(x[i]).hex(), len(err)))
    return float(err[i])


def test_sincos_2pi_accuracy(oracle):
    u = dp.input_set("sincos_2pi")
    got = oracle_out(oracle, "sincos_2pi").astype(np.float64)
    a = 2.0 * np.pi * u.astype(np.float64)
    tc, ts = np.cos(a), np.sin(a)
    err = np.maximum(np.abs(got[:, 0] - tc), np.abs(got[:, 1] - ts))
    # the larger component lies in [sqrt(1/2), 1]: its binade's ulp is 2^-24 (2^-23 only where it is exactly 1)
    ulp = _ulp32(np.maximum(np.abs(tc), np.abs(ts)))
    worst = _report("sincos_2pi", err / ulp, u, "ulp of the larger component's binade")
    _report("sincos_2pi", err, u, "absolute")
    assert worst <= 1.7
    # the axes are exact
    for k, cs in ((0, (1.0, 0.0)), (1 << 21, (0.0, 1.0)), (1 << 22, (-1.0, 0.0)), (3 << 21, (0.0, -1.0))):
        assert tuple(got[k]) == cs, (k, got[k])        # (-0.0 == 0.0: the sign of a zero component is not part of this)


def test_sincosf_accuracy(oracle):
    x = dp.input_set("sincosf")
    got = oracle_out(oracle, "sincosf").astype(np.float64)
    m = dp.in_domain("sincosf", x)
    t = x[m].astype(np.float64)
    err = np.maximum(np.abs(got[m, 0] - np.cos(t)), np.abs(got[m, 1] - np.sin(t)))
    worst = _report("sincosf", err, x[m], "absolute")
    assert worst <= 2.0e-7 + np.pi * 2.0 ** -23


def test_logf_accuracy_whole_set(oracle):
    x = dp.input_set("logf")
    got = oracle_out(oracle, "logf").astype(np.float64)
    m = dp.in_domain("logf", x)
    ref = np.log(x[m].astype(np.float64))
    err = np.abs(got[m] - ref)
    _report("logf", err / _ulp32(np.where(ref == 0, 1.0, ref)), x[m], "ulp")
    worst = _report("logf", err / np.maximum(1.0, np.abs(ref)), x[m], "relative to max(1, |ref|)")
    assert worst <= 4e-7
    assert got[m][x[m] == 1.0] == 0.0


def _expf_errors(x, got):
    """errors of e^x in ulp for normal results (an overflowed result counts as 2^128, and is right where the exact value is
    not below that), in units of 2^-149 for subnormal ones"""
    ref = np.exp(x.astype(np.float64))
    normal = ref >= 2.0 ** -126
    g = np.where(np.isinf(got), 2.0 ** 128, got)
    err_n = np.abs(g - ref) / _ulp32(ref)
    err_n = np.where(np.isinf(got) & (ref >= 2.0 ** 128), 0.0, err_n)
    err_s = np.abs(got - ref) / 2.0 ** -149
    return normal, err_n, err_s


def test_expf_accuracy(oracle):
    x = dp.input_set("expf")
    m = dp.in_domain("expf", x)
    got = oracle_out(oracle, "expf").astype(np.float64)[m]
    x = x[m]
    assert np.all(got >= 0) and not np.any(np.isnan(got))
    normal, err_n, err_s = _expf_errors(x, got)
    wn = _report("expf, normal results", err_n[normal], x[normal], "ulp")
    ws = _report("expf, subnormal results", err_s[~normal], x[~normal], "units of 2^-149")
    assert (~normal).sum() > 1000       # the set reaches the subnormal results
    assert wn <= 2.0
    assert ws <= 1.0
    assert got[x == 0].tolist() == [1.0] * int((x == 0).sum())


def test_cbrt01_accuracy_and_range(oracle):
    x = dp.input_set("cbrt01")
    got = oracle_out(oracle, "cbrt01")
    n = 1 << 23
    assert got[0] == 0.0 and x[0] == 0.0
    # sqrtf(1 - cbrt01(u1^2)) has no guard: never above 1, and never decreasing in g
    assert got.max() <= 1.0
    assert got[n] == 1.0                                        # cbrt01(1.0)
    assert np.all(np.diff(got[:n]) >= 0)
    pos = x > 0
    xd = x[pos].astype(np.float64)
    ref = np.cbrt(xd)
    err = np.abs(got[pos].astype(np.float64) - ref) / ref
    bound = 4e-7 * np.maximum(1.0, np.abs(np.log(xd))) / 3.0 + 3.0 * 2.0 ** -23
    _report("cbrt01, the squared draws", err[:n - 1], x[pos][:n - 1], "relative")
    _report("cbrt01", err, x[pos], "relative")
    worst = _report("cbrt01", err / bound, x[pos], "of its bound")
    assert worst <= 1.0


_MP_SUBSET = 20000


def _fp64_check(oracle, fn, mp_fn, exact):
    """relative error of an fp64 function against mpmath at 40 digits: a fixed seeded subset of the 2^20 spread arguments and
    every listed neighbourhood; where the exact result is 0 the function must return 0"""
    import mpmath
    x = dp.input_set(fn)
    got = oracle_out(oracle, fn)
    pick = np.sort(np.random.default_rng(7).choice(1 << 20, _MP_SUBSET, replace=False))
    idx = np.concatenate([pick, np.arange(1 << 20, len(x))])
    idx = idx[dp.in_domain(fn, x[idx])]
    assert len(idx) >= _MP_SUBSET + 100
    worst, where = 0.0, None
    with mpmath.workdps(40):
        for i in idx:
            xi = float(x[i])
            ref = mp_fn(mpmath.mpf(xi))
            g = float(got[i])
            if ref == 0:
                assert g == 0.0, (fn, xi, g)
                continue
            err = float(abs((mpmath.mpf(g) - ref) / ref))
            if err > worst:
                worst, where = err, xi
    print("%s: worst relative error %.4g at argument %r (%s), %d arguments" % (fn, worst, where, where.hex(), len(idx)))
    for xi, v in exact:
        k = np.flatnonzero(x == xi)
        assert len(k) > 0 and np.all(got[k] == v) and not np.any(np.signbit(got[k])), (fn, xi, got[k])
    assert worst < 1e-15
    return worst


def test_cospi_d_accuracy(oracle):
    import mpmath
    # cos(pi / 2) is the one exact zero; at 40 digits mpmath's pi / 2 is off by 1e-41 and its cosine with it
    _fp64_check(oracle, "cospi_d", lambda u: mpmath.mpf(0) if u == 0.5 else mpmath.cos(mpmath.pi * u),
                exact=((0.5, 0.0), (0.0, 1.0)))


def test_acos_d_accuracy(oracle):
    import mpmath
    _fp64_check(oracle, "acos_d", mpmath.acos, exact=((1.0, 0.0),))


def test_log_d_accuracy(oracle):
    import mpmath
    _fp64_check(oracle, "log_d", mpmath.log, exact=((1.0, 0.0),))


def test_pcg_against_integer_arithmetic(oracle):
    """the oracle's PCG32 rows against Python integers: seeding, the three kinds of draw, advance(delta) by the closed form
    M^n s + inc (M^n - 1)/(M - 1), and two discarded draws (what the device's pcg_skip2 replaces by one jump)"""
    M, mask = 0x5851F42D4C957F2D, (1 << 64) - 1
    x = dp.input_set("pcg").reshape(-1, 3)
    out = oracle_out(oracle, "pcg")
    rows = np.concatenate([np.arange(0, len(x), 97), np.arange(len(x) - len(dp.PCG_DELTAS), len(x))])

    def draw(s, inc):
        xs = (((s >> 18) ^ s) >> 27) & 0xFFFFFFFF
        rot = s >> 59
        return (s * M + inc) & mask, ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF

    for r in rows:
        initstate, initseq, delta = (int(v) for v in x[r])
        inc = ((initseq << 1) | 1) & mask
        s, _ = draw(0, inc)
        s, _ = draw((s + initstate) & mask, inc)
        exp = [s, inc]
        s, u = draw(s, inc)
        exp.append(u)
        s, u = draw(s, inc)
        exp.append(int(np.float32(np.uint32((u >> 9) | 0x3F800000).view(np.float32) - np.float32(1.0)).view(np.uint32)))
        s, u = draw(s, inc)
        exp.append(int(np.float64(np.uint64((u << 20) | 0x3FF0000000000000).view(np.float64) - 1.0).view(np.uint64)))
        exp.append(s)
        mn = pow(M, delta, (M - 1) << 64)
        s = ((mn * s) + inc * ((mn - 1) // (M - 1))) & mask
        exp.append(s)
        s, _ = draw(s, inc)
        s, _ = draw(s, inc)
        exp.append(s)
        assert [int(v) for v in out[r]] == exp, (r, initstate, initseq, delta)
    # the canonical pair (42, 54): first output of the known-answer vector
    canon = out[len(x) - len(dp.PCG_DELTAS)]
    assert int(canon[2]) == 0xA15C02B7


# ---- (c) out-of-domain values, pinned ------------------------------------------------------------------------------------
LN2_F = float.fromhex("0x1.62e430p-1")      # the log's fp32 ln 2


def _at(oracle, fn, value):
    x = dp.input_set(fn)
    v = np.asarray(value, x.dtype)
    k = np.flatnonzero(_bits(x) == _bits(v.reshape(1))[0])
    assert len(k) > 0, (fn, value)
    return oracle_out(oracle, fn)[k[0]]


def test_out_of_domain_values(oracle):
    # logf: +0 takes the subnormal path with a zero mantissa (e = -150), +inf is read as 1.0 x 2^128 -- finite values both
    assert _at(oracle, "logf", 0.0) == np.float32(-150.0 * LN2_F)
    assert _at(oracle, "logf", np.inf) == np.float32(128.0 * LN2_F)
    assert abs(float(_at(oracle, "logf", np.inf)) - 88.7228) < 1e-4
    assert np.isnan(_at(oracle, "expf", np.nan))
    assert _at(oracle, "expf", np.inf) == np.inf
    z = _at(oracle, "expf", -np.inf)
    assert z == 0.0 and not np.signbit(z)
    assert _at(oracle, "expf", -0.0) == 1.0 and _at(oracle, "expf", 0.0) == 1.0
    # a NaN angle is the angle 0
    assert tuple(_at(oracle, "sincosf", np.nan)) == (1.0, 0.0)
    for v in (np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), 2.0, -2.0, np.inf, -np.inf, np.nan):
        assert np.isnan(_at(oracle, "acos_d", v)), v
    assert _at(oracle, "log_d", 0.0) == -np.inf and _at(oracle, "log_d", -0.0) == -np.inf
    assert np.isnan(_at(oracle, "log_d", -1.5)) and np.isnan(_at(oracle, "log_d", -np.inf)) and np.isnan(_at(oracle, "log_d", np.nan))
    assert _at(oracle, "log_d", np.inf) == np.inf


def test_green_sampler_trial_at_radius_zero(oracle):
    """sampleSource's rejection trial with r == 0 (wost_walk.h / wost_oracle.c): logf(R_B / 0) = logf(+inf) is the finite
    128 ln 2, so the trial is accepted iff u < (128 ln 2) * 4 / 1.5 / R_B = 236.59 / R_B -- always (u < 1) for R_B up to
    236.59, with that probability beyond; a rejected trial just draws again."""
    f = np.float32
    L = f(_at(oracle, "logf", np.inf))
    two_pi = f(6.28318530717958647693)

    def ratio(R_B):
        R_B = f(R_B)
        norm, bound = f(f(R_B * R_B) / f(4.0)), f(f(1.5) / R_B)
        pdf = f(f(L / two_pi) / norm)
        return f(f(pdf / f(f(1.0) / two_pi)) / bound)

    largest_u = f(1.0) - f(2.0 ** -23)                 # pcg_next_float's largest value
    for R_B in (1e-3, 1.0, 100.0, 236.0):
        assert largest_u < ratio(R_B)
    for R_B in (237.0, 500.0, 1e4):
        assert ratio(R_B) < largest_u
        assert abs(float(ratio(R_B)) * R_B / 236.594 - 1.0) < 1e-4
    assert math.isclose(float(L) * 4.0 / 1.5, 236.594, rel_tol=1e-5)
