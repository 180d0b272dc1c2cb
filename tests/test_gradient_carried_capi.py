"""The carried gradient list in the C-ABI (wost_gradient_points_carry, _carry_dev, _more, _more_dev, _carried, _adaptive,
_adaptive_dev, _restart, _progress and their wost3_ forms) without a GPU: the eighteen names exist, include/wost.h declares them,
Python knows their prototypes and the two structs, and every argument that can be refused before the handle is read is refused
with WOST_ERR_INVALID and a message that names the quantity, the outputs untouched.  (The handle is a block of zeroed memory:
none of these refusals may read it.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_ARGS = {"gradient_points_carry": 9, "gradient_points_carry_dev": 10, "gradient_points_more": 4, "gradient_points_more_dev": 5,
          "gradient_points_carried": 2, "gradient_points_adaptive": 4, "gradient_points_adaptive_dev": 5, "gradient_points_restart": 1,
          "gradient_points_progress": 3}
PREFIXES = ["wost_", "wost3_"]
NAMES = [pre + f for pre in PREFIXES for f in N_ARGS]
WOST_ERR_INVALID = -1


def _fake_handle():
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


class _Outputs:
    """the five arrays of a wost_gradient_carried_out for 4 points, filled with -1"""

    def __init__(self, dim):
        self.arrays = {"grad": np.full(4 * dim * 3, -1.0, np.float32), "grad_stderr": np.full(4 * dim * 3, -1.0, np.float32),
                       "field_rgb": np.full(12, -1.0, np.float32), "radius": np.full(4, -1.0, np.float32), "batches": np.full(4, -1, np.int32)}

    def struct(self, capi):
        return capi.GradientCarriedOut(*[self.arrays[f[0]].ctypes.data for f in capi.GradientCarriedOut._fields_])

    def untouched(self):
        return all(np.all(a == -1) for a in self.arrays.values())


def test_there_are_eighteen_names():
    assert len(NAMES) == len(set(NAMES)) == 18


def test_the_two_structs_have_the_stated_fields_and_sizes():
    from elaina_amd import capi
    assert [f[0] for f in capi.GradientCarriedOut._fields_] == ["grad", "grad_stderr", "field_rgb", "radius", "batches"]
    assert C.sizeof(capi.GradientCarriedOut) == 5 * C.sizeof(C.c_void_p)
    assert [(f[0], f[1]) for f in capi.GradientAdaptive._fields_] == [("min_batches", C.c_int32), ("max_batches", C.c_int32),
                                                                       ("abs_tol", C.c_float), ("rel_tol", C.c_float)]
    assert C.sizeof(capi.GradientAdaptive) == 16


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_are_exported_declared_and_prototyped(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == N_ARGS[name.split("_", 1)[1]]
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    m = re.search(r"^int %s\((wost3?_handle h[^;]*)\);" % name, header, re.M | re.S)
    assert m, name
    assert m.group(1).count(",") + 1 == N_ARGS[name.split("_", 1)[1]], m.group(1)
    assert m.group(1).startswith("wost3_handle" if name.startswith("wost3_") else "wost_handle")


@pytest.mark.parametrize("pre", PREFIXES)
def test_a_bind_is_checked_in_the_documented_order_before_the_handle_is_read(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    dim = 2 if pre == "wost_" else 3
    pts = np.zeros((4, dim), np.float32)
    pts[2, 1] = np.nan          # (the host form's scan comes last)
    p = capi._fp(pts)
    host, dev = getattr(lib, pre + "gradient_points_carry"), getattr(lib, pre + "gradient_points_carry_dev")
    T = 1 << 28
    # (handle, points, n, batch_walks, round_stride, max_rounds, seed_base, walk_seed_base, seed_width) -> the word of the
    # refusal; every row breaks the rule it names and, as far as one call can, the rules after it, so the order shows
    rows = [
        ((None, p, -1, 1, -2, 0, -1, -1, 0), b"null"),
        ((handle, None, -1, 1, -2, 0, -1, -1, 0), b"negative"),
        ((handle, None, 4, 1, 3, 0, -1, -1, 0), b"null"),
        ((handle, p, 4, 1, 3, 0, -1, -1, 0), b"seed_width"),
        ((handle, p, 4, 1, 3, 0, -1, -1, -16), b"seed_width"),
        ((handle, p, 4, 1, 3, 0, -1, 5, 16), b"seed_base"),
        ((handle, p, 4, 1, 3, 0, 5, -1, 16), b"walk_seed_base"),
        ((handle, p, 4, 1, 3, 0, T, T, 16), b"batch_walks"),
        ((handle, p, 4, -7, 3, 0, T, T, 16), b"batch_walks"),
        ((handle, p, 4, 8, 3, 0, T, T, 16), b"round_stride"),
        ((handle, p, 4, 8, 4, 0, T, T, 16), b"max_rounds"),
        ((handle, p, 4, 8, 4, -2, T, T, 16), b"max_rounds"),
        # the direction seeds end at (2^28 - 7) + 1 * 4 + 4 = 2^28 + 1
        ((handle, p, 4, 8, 4, 2, T - 7, T, 16), b"seed_base + (max_rounds - 1) * round_stride + n"),
        # ... and in 64 bits: 2^31 - 1 rounds of stride 2^31 - 1
        ((handle, p, 4, 8, (1 << 31) - 1, (1 << 31) - 1, 0, T, 16), b"seed_base + (max_rounds - 1) * round_stride + n"),
        # the walk seeds end at (2^28 - 63) + (1 * 4 + 4) * 8 = 2^28 + 1
        ((handle, p, 4, 8, 4, 2, 0, T - 63, 16), b"walk_seed_base + ((max_rounds - 1) * round_stride + n) * batch_walks"),
        # ... and in 64 bits: a span of 2^24 points times 256 walks is 2^32, which is 0 in 32 bits
        ((handle, p, 4, 256, 1 << 23, 3, 0, 0, 16), b"walk_seed_base + ((max_rounds - 1) * round_stride + n) * batch_walks"),
        # [0, 8) and [7, 71); [100, 108) and [40, 104)
        ((handle, p, 4, 8, 4, 2, 0, 7, 16), b"overlap"),
        ((handle, p, 4, 8, 4, 2, 100, 40, 16), b"overlap"),
    ]
    for k, ((h, pp, n, S, stride, rounds, base, walk, width), word) in enumerate(rows):
        assert host(h, pp, n, S, stride, rounds, base, walk, width) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
        d = None if pp is None else C.c_void_p(pts.ctypes.data)
        assert dev(h, d, n, S, stride, rounds, base, walk, width, None) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    # the seed ranges may end at 2^28 exactly and may touch: then the host form's scan finds the bad point
    assert host(handle, p, 4, 8, 4, 2, T - 8, T - 72, 16) == WOST_ERR_INVALID and b"point 2 " in lib.wost_last_error(), lib.wost_last_error()
    pts[1, 0] = np.inf
    assert host(handle, p, 4, 8, 4, 2, 0, 8, 16) == WOST_ERR_INVALID and b"point 1 " in lib.wost_last_error(), lib.wost_last_error()


@pytest.mark.parametrize("pre", PREFIXES)
def test_an_empty_bind_is_ok(pre):
    """n == 0 releases the list; a handle that has none has nothing to release, and no device is asked for"""
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    assert getattr(lib, pre + "gradient_points_carry")(handle, None, 0, 8, 0, 1, 0, 0, 16) == 0
    assert getattr(lib, pre + "gradient_points_carry_dev")(handle, None, 0, 8, 0, 1, 1 << 28, 0, 16, None) == 0
    n, r = C.c_int32(-5), C.c_int32(-5)
    assert getattr(lib, pre + "gradient_points_progress")(handle, C.byref(n), C.byref(r)) == 0 and (n.value, r.value) == (0, 0)


@pytest.mark.parametrize("pre", PREFIXES)
def test_null_pointers_are_refused(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    o = _Outputs(2 if pre == "wost_" else 3)
    go = o.struct(capi)
    no_grad = o.struct(capi)
    no_grad.grad = None
    a = capi.GradientAdaptive(3, 12, 0.1, 0.0)
    st = capi.Stats()
    n = C.c_int32(-5)
    f = lambda name: getattr(lib, pre + "gradient_points_" + name)
    calls = [
        lambda: f("more")(None, None, C.byref(go), C.byref(st)),
        lambda: f("more")(handle, None, None, C.byref(st)),
        lambda: f("more")(handle, None, C.byref(no_grad), C.byref(st)),
        lambda: f("more_dev")(None, None, C.byref(go), None, C.byref(st)),
        lambda: f("more_dev")(handle, None, C.byref(no_grad), None, C.byref(st)),
        lambda: f("carried")(None, C.byref(go)),
        lambda: f("carried")(handle, None),
        lambda: f("carried")(handle, C.byref(no_grad)),
        lambda: f("adaptive")(None, C.byref(a), C.byref(go), C.byref(st)),
        lambda: f("adaptive")(handle, None, C.byref(go), C.byref(st)),
        lambda: f("adaptive")(handle, C.byref(a), None, C.byref(st)),
        lambda: f("adaptive")(handle, C.byref(a), C.byref(no_grad), C.byref(st)),
        lambda: f("adaptive_dev")(None, C.byref(a), C.byref(go), None, C.byref(st)),
        lambda: f("adaptive_dev")(handle, None, C.byref(go), None, C.byref(st)),
        lambda: f("adaptive_dev")(handle, C.byref(a), C.byref(no_grad), None, C.byref(st)),
        lambda: f("restart")(None),
        lambda: f("progress")(None, C.byref(n), C.byref(n)),
        lambda: f("progress")(handle, None, C.byref(n)),
        lambda: f("progress")(handle, C.byref(n), None),
    ]
    for k, call in enumerate(calls):
        assert call() == WOST_ERR_INVALID and b"null" in lib.wost_last_error(), (k, lib.wost_last_error())
    assert o.untouched() and n.value == -5


BAD_ADAPTIVE = [((1, 12, 0.1, 0.0), b"min_batches"), ((0, 12, 0.1, 0.0), b"min_batches"), ((2, 0, 0.1, 0.0), b"max_batches"),
                ((2, -3, 0.1, 0.0), b"max_batches"), ((2, 12, -0.1, 0.0), b"abs_tol"), ((2, 12, 0.1, -1.0), b"rel_tol"),
                ((2, 12, float("nan"), 0.0), b"abs_tol"), ((2, 12, 0.0, float("inf")), b"rel_tol")]


@pytest.mark.parametrize("pre", PREFIXES)
@pytest.mark.parametrize("settings,word", BAD_ADAPTIVE, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else None)
def test_adaptive_settings_are_refused_before_the_handle_is_read(pre, settings, word):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    o = _Outputs(2 if pre == "wost_" else 3)
    go = o.struct(capi)
    a = capi.GradientAdaptive(*settings)
    st = capi.Stats()
    assert getattr(lib, pre + "gradient_points_adaptive")(handle, C.byref(a), C.byref(go), C.byref(st)) == WOST_ERR_INVALID
    assert word in lib.wost_last_error(), lib.wost_last_error()
    assert getattr(lib, pre + "gradient_points_adaptive_dev")(handle, C.byref(a), C.byref(go), None, C.byref(st)) == WOST_ERR_INVALID
    assert word in lib.wost_last_error(), lib.wost_last_error()
    assert o.untouched()


@pytest.mark.parametrize("pre", PREFIXES)
def test_calls_without_a_bound_list_say_so(pre):
    """a zeroed handle has no list: the calls that need one are refused once their own arguments have passed"""
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    o = _Outputs(2 if pre == "wost_" else 3)
    go = o.struct(capi)
    a = capi.GradientAdaptive(3, 12, 0.1, 0.0)
    st = capi.Stats()
    f = lambda name: getattr(lib, pre + "gradient_points_" + name)
    calls = [
        lambda: f("more")(handle, None, C.byref(go), C.byref(st)),
        lambda: f("more_dev")(handle, None, C.byref(go), None, C.byref(st)),
        lambda: f("carried")(handle, C.byref(go)),
        lambda: f("adaptive")(handle, C.byref(a), C.byref(go), C.byref(st)),
        lambda: f("adaptive_dev")(handle, C.byref(a), C.byref(go), None, C.byref(st)),
        lambda: f("restart")(handle),
    ]
    for k, call in enumerate(calls):
        assert call() == WOST_ERR_INVALID and b"no gradient list is bound" in lib.wost_last_error(), (k, lib.wost_last_error())
    assert o.untouched()
