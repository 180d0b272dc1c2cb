"""Helper of tests/test_device_math.py: the ctypes binding of the device probe (tests/probe/wost_probe.hip, built into
elaina_amd/lib/libwost_probe.so by elaina_amd.build.build_probe()) and the fixed, seeded input sets that both layers of that test
use -- the device against the oracle bit for bit, and the oracle against a high-precision reference."""
import ctypes as C
import functools
import os

import numpy as np

from oracle.oracle import PROBE_FUNCTIONS, probe_arrays

_lib = None


def load():
    """libwost_probe.so; a missing library is an error (run `python __graft_entry__.py`)"""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (one HIP runtime in the process: torch's, loaded first -- DESIGN.md "runtime")
        from elaina_amd import build as b
        if not os.path.exists(b.PROBE_PATH):
            raise RuntimeError("libwost_probe.so is missing (%s): run `python __graft_entry__.py`" % b.PROBE_PATH)
        _lib = C.CDLL(b.PROBE_PATH)
        _lib.wost_probe_run.restype = C.c_int
        _lib.wost_probe_run.argtypes = [C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.wost_order_probe_open.restype = C.c_int
        _lib.wost_order_probe_open.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
        _lib.wost_order_probe_run.restype = C.c_int
        _lib.wost_order_probe_run.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
        _lib.wost_order_probe_close.restype = C.c_int
        _lib.wost_order_probe_close.argtypes = [C.c_void_p]
    return _lib


def device_probe(fn, x, device=0):
    """one device function (a name of PROBE_FUNCTIONS) over an array of arguments"""
    num, a, n, out = probe_arrays(fn, x)
    rc = load().wost_probe_run(device, num, a.ctypes.data, n, out.ctypes.data)
    if rc != 0:
        raise RuntimeError("wost_probe_run(%s): hipError_t %d" % (fn, rc))
    return out


ORDER_SENTINEL = 0xFFFFFFFF
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1


class WalkOrderProbe:
    """one WalkOrder of the product (csrc/wost_order.h) for `cap` walkers, through tests/probe/wost_order_probe.hip: the scratch
    is sized once and serves every run, as a handle's does"""

    BY_DISTANCE, BY_ESTIMATE = 0, 1

    def __init__(self, cap, device=0):
        self.lib, self.cap, self._h = load(), int(cap), C.c_void_p()
        rc = self.lib.wost_order_probe_open(device, self.cap, C.byref(self._h))
        if rc != 0:
            raise RuntimeError("wost_order_probe_open(%d): hipError_t %d" % (self.cap, rc))

    def run(self, which, keys):
        """order_by_distance / order_by_estimate on a float32 array -> (what the function returned, all cap entries of the buffer
        *order_out points into, all cap entries of the other value buffer); both buffers held ORDER_SENTINEL before the run"""
        keys = np.ascontiguousarray(keys, dtype=np.float32)
        rc = C.c_int32(-1)
        out, other = np.zeros(self.cap, np.uint32), np.zeros(self.cap, np.uint32)
        e = self.lib.wost_order_probe_run(self._h, which, keys.ctypes.data, len(keys), C.byref(rc), out.ctypes.data, other.ctypes.data)
        if e != 0:
            raise RuntimeError("wost_order_probe_run: error %d of the probe's own calls" % e)
        return rc.value, out, other

    def by_distance(self, d2):
        return self.run(self.BY_DISTANCE, d2)

    def by_estimate(self, est):
        return self.run(self.BY_ESTIMATE, est)

    def close(self):
        if self._h:
            self.lib.wost_order_probe_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- building blocks ------------------------------------------------------------------------------------------------------
def f32_from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def f64_from_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def _around(x, k, ftype, itype, nbits):
    """the k floats on either side of x and x itself, in value order; steps through zero into the other sign.  Floats are
    ordered like the integers sign * magnitude-bits."""
    top = 1 << (nbits - 1)
    b = int(np.asarray(x, dtype=ftype).view(itype))
    key = -(b & (top - 1)) if b & top else b
    keys = [key + d for d in range(-k, k + 1)]
    bits = [(top | -q) if q < 0 else q for q in keys]
    return np.asarray(bits, dtype=itype).view(ftype)


def around32(x, k=64):
    return _around(x, k, np.float32, np.uint32, 32)


def around64(x, k=4):
    return _around(x, k, np.float64, np.uint64, 64)


PI_F = np.float32(np.pi)
F32_TINY = f32_from_bits(0x00000001)            # smallest subnormal
F32_SUB_MAX = f32_from_bits(0x007fffff)         # largest subnormal
F32_MIN_NORMAL = f32_from_bits(0x00800000)
SQRT2_SWITCH_F = np.float32(float.fromhex("0x1.6a09e6p+0"))
SQRT2_SWITCH_D = 1.4142135623730951
LN2 = 0.6931471805599453094


# the points where the k of the exponential steps: x = (m + 1/2) ln 2, 32 values of m over the whole range of k (-150 ... 128)
EXP_K_STEPS = np.unique(np.round(np.linspace(-150, 127, 32))).astype(np.int64)
assert len(EXP_K_STEPS) == 32

PCG_DELTAS = (0, 1, 2, 3, 1 << 32, (1 << 62) - 1)


@functools.lru_cache(maxsize=None)
def input_set(fn):
    """the whole input set of one probe function: a read-only array, the same on every call"""
    rng = np.random.default_rng(20240 + PROBE_FUNCTIONS[fn][0])
    if fn == "sincos_2pi":
        x = np.arange(1 << 23, dtype=np.float32) * np.float32(2.0 ** -23)
    elif fn == "sincosf":
        parts = [np.clip(rng.uniform(-np.pi, np.pi, 1 << 20).astype(np.float32), -PI_F, PI_F),
                 around32(PI_F, 2), around32(-PI_F, 2), f32_from_bits([0x00000000, 0x80000000])]
        parts += [around32(np.float32(k * np.pi / 4)) for k in range(-4, 5)]
        # negative arguments whose turn fraction u is so small that u + 1 rounds to 1 (then u = 0): around u = -2^-25, the tie,
        # around u = -2^-24, the first that does not, and far below
        parts += [around32(np.float32(-2.0 * np.pi * 2.0 ** -25)), around32(np.float32(-2.0 * np.pi * 2.0 ** -24)),
                  np.asarray([-1e-8, -1e-10, -1e-20, -1e-38, -1e-44], np.float32), -F32_TINY.reshape(1)]
        parts += [np.asarray([np.nan], np.float32)]
        x = np.concatenate(parts)
    elif fn == "logf":
        mant = rng.integers(0, 1 << 23, size=(255, 4096), dtype=np.uint32)
        mant[0][mant[0] == 0] = 1                                          # exponent field 0: subnormals, never +0
        spread = f32_from_bits((np.arange(255, dtype=np.uint32)[:, None] << 23) | mant).ravel()
        parts = [spread, around32(1.0, 1 << 16)]
        parts += [around32(SQRT2_SWITCH_F * np.float32(s)) for s in (0.125, 1.0, 32.0)]
        parts += [np.asarray([F32_TINY, F32_SUB_MAX, F32_MIN_NORMAL], np.float32)]
        parts += [np.asarray([0.0, np.inf], np.float32)]                   # out of domain, reachable by a walk
        x = np.concatenate(parts)
    elif fn == "expf":
        parts = [rng.uniform(-104.0, 88.8, 1 << 20).astype(np.float32)]
        parts += [around32(np.float32(c)) for c in (-104.0, -87.34, 0.0, 88.72, 88.8)]
        parts += [around32(np.float32((float(m) + 0.5) * LN2)) for m in EXP_K_STEPS]
        parts += [f32_from_bits([0x00000000, 0x80000000]), np.asarray([np.inf, -np.inf, np.nan], np.float32)]
        x = np.concatenate(parts)
    elif fn == "cbrt01":
        g = np.arange(1 << 23, dtype=np.float32) * np.float32(2.0 ** -23)
        x = np.concatenate([g * g, np.asarray([1.0, F32_TINY], np.float32)])     # g * g in fp32, as the sampler forms it
    elif fn == "cospi_d":
        j = np.arange(2, 53)
        parts = [rng.random(1 << 20), 0.5 + 2.0 ** -j, 0.5 - 2.0 ** -j, around64(0.5), around64(0.25),
                 np.asarray([0.0, np.nextafter(1.0, 0.0), 2.0 ** -1074, 2.0 ** -1022, 1e-300, 1e-17])]
        x = np.concatenate(parts)
    elif fn == "acos_d":
        j = np.arange(1, 54)
        parts = [rng.uniform(-1.0, 1.0, 1 << 20), 1.0 - 2.0 ** -j, -1.0 + 2.0 ** -j, around64(0.5), around64(-0.5),
                 around64(0.0), np.asarray([1.0, -1.0, 1e-300, -1e-300])]
        parts += [np.asarray([np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), 2.0, -2.0, np.inf, -np.inf, np.nan])]  # out of domain
        x = np.concatenate(parts)
    elif fn == "log_d":
        j = np.arange(1, 53)
        parts = [np.exp2(rng.uniform(-60.0, 60.0, 1 << 20)), 1.0 + 2.0 ** -j, 1.0 - 2.0 ** -j, around64(1.0)]
        parts += [around64(SQRT2_SWITCH_D * s, 64) for s in (2.0 ** -40, 1.0, 2.0 ** 17)]
        parts += [f64_from_bits(rng.integers(1, 1 << 52, 4096, dtype=np.uint64)),                          # subnormals
                  np.asarray([2.0 ** -1074, np.nextafter(2.0 ** -1022, 0.0), 2.0 ** -1022, np.finfo(np.float64).max])]
        parts += [np.asarray([0.0, -0.0, np.inf, -1.5, -np.inf, np.nan])]                                 # out of domain
        x = np.concatenate(parts)
    elif fn == "pcg":
        pairs = rng.integers(0, 1 << 64, size=(4096, 2), dtype=np.uint64)
        pairs = np.concatenate([pairs, np.asarray([[42, 54]], np.uint64)])        # the canonical pair of test_pcg32_canonical_kat
        x = np.asarray([(s, q, d) for s, q in pairs.tolist() for d in PCG_DELTAS], dtype=np.uint64)
    elif fn == "proposal_r":
        # kappa = exp(clamp(raw, -10, 15)) in the mixture; the Taylor switch at 1e-5, zero, subnormal, huge and non-finite values
        parts = [np.exp(rng.uniform(-10.0, 15.0, 1 << 16)).astype(np.float32), around32(np.float32(1e-5)), around32(0.0, 4)[4:],
                 np.asarray([1e-3, 1.0, 3.75, 1e10, 1e19, 1e20, 3e38, np.inf, np.nan], np.float32)]
        x = np.concatenate(parts)
    else:
        raise KeyError(fn)
    x = np.ascontiguousarray(x, dtype=PROBE_FUNCTIONS[fn][1])
    x.setflags(write=False)
    return x


def in_domain(fn, x):
    """mask of the arguments the function is specified for (the accuracy layer leaves the others to explicit asserts)"""
    if fn in ("sincosf",):
        return ~np.isnan(x)
    if fn == "logf":
        return (x > 0) & np.isfinite(x)
    if fn == "expf":
        return np.isfinite(x)
    if fn == "acos_d":
        return (x >= -1.0) & (x <= 1.0)
    if fn == "log_d":
        return (x > 0) & np.isfinite(x)
    return np.ones(x.shape, bool)
