"""The exit list of the gradient in the C-ABI (wost_exits_walk_gradient, _walk_gradient_dev, _gradient_records, _apply_gradient,
_apply_gradient_dev, _adjoint_gradient, _adjoint_gradient_dev and their wost3_ forms) without a GPU: the fourteen names exist,
include/wost.h declares them, Python knows their prototypes and the struct, and every argument that can be refused before the
handle is read is refused with WOST_ERR_INVALID, in the order of the header, with a message that names the quantity and the
outputs untouched.  (The handle is a block of zeroed memory: none of these refusals may read more of it than the fact that it
holds no list.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_ARGS = {"exits_walk_gradient": 8, "exits_walk_gradient_dev": 9, "exits_gradient_records": 2, "exits_apply_gradient": 6,
          "exits_apply_gradient_dev": 7, "exits_adjoint_gradient": 4, "exits_adjoint_gradient_dev": 5}
PREFIXES = ["wost_", "wost3_"]
NAMES = [pre + f for pre in PREFIXES for f in N_ARGS]
WOST_ERR_INVALID = -1


def _fake_handle():
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


def test_there_are_fourteen_names_and_the_struct_has_the_stated_fields():
    from elaina_amd import capi
    assert len(NAMES) == len(set(NAMES)) == 14
    assert [f[0] for f in capi.ExitGradientRecords._fields_] == ["radius", "dirs", "first_pts"]
    assert C.sizeof(capi.ExitGradientRecords) == 3 * C.sizeof(C.c_void_p)
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    m = re.search(r"typedef struct wost_exit_gradient_records \{(.*?)\} wost_exit_gradient_records;", header, re.S)
    assert re.findall(r"\*(\w+);", m.group(1)) == ["radius", "dirs", "first_pts"]
    assert "Exit lists of the gradient" in header and header.index("Exit lists of the gradient") > header.index("/* Exit lists (DESIGN 4.3h)")


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
def test_a_walk_is_checked_in_the_documented_order_before_the_handle_is_read(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    dim = 2 if pre == "wost_" else 3
    pts = np.zeros((4, dim), np.float32)
    pts[2, 1] = np.nan          # (the host form's scan comes last)
    p = capi._fp(pts)
    host, dev = getattr(lib, pre + "exits_walk_gradient"), getattr(lib, pre + "exits_walk_gradient_dev")
    T = 1 << 28
    # (handle, points, n, walks, seed_base, walk_seed_base, seed_width) -> the word of the refusal; every row breaks the rule it
    # names and, as far as one call can, the rules after it, so the order shows
    rows = [
        ((None, p, -1, 1, -1, -1, 0), b"null"),
        ((handle, None, -1, 1, -1, -1, 0), b"negative"),
        ((handle, None, 4, 1, -1, -1, 0), b"null"),
        ((handle, p, 4, 1, -1, -1, 0), b"walks must be at least 2"),
        ((handle, p, 4, -3, -1, -1, 0), b"walks must be at least 2"),
        ((handle, p, 4, 8, -1, -1, 0), b"seed_width"),
        ((handle, p, 4, 8, -1, -1, -16), b"seed_width"),
        ((handle, p, 4, 8, -1, T, 16), b"must be >= 0"),
        ((handle, p, 4, 8, T, -1, 16), b"must be >= 0"),
        # the directions' seeds end at (2^28 - 3) + 4 = 2^28 + 1 -- and so would the walks'
        ((handle, p, 4, 8, T - 3, T - 31, 16), b"seed_base + n must be at most 2^28"),
        # the walks' seeds end at (2^28 - 31) + 4 * 8 = 2^28 + 1, and their range holds the directions'
        ((handle, p, 4, 8, T - 20, T - 31, 16), b"walk_seed_base + n * walks"),
        # ... and in 64 bits: 2^24 points times 256 walks is 2^32, which is 0 in 32 bits
        ((handle, p, 1 << 24, 256, 0, 0, 16), b"walk_seed_base + n * walks"),
        # the ranges [10, 14) and [13, 45), [40, 44) and [13, 45), [0, 4) and [0, 32) overlap
        ((handle, p, 4, 8, 10, 13, 16), b"overlap"),
        ((handle, p, 4, 8, 40, 13, 16), b"overlap"),
        ((handle, p, 4, 8, 0, 0, 16), b"overlap"),
    ]
    st = capi.Stats()
    st.walk_steps = 5
    for k, ((h, pp, n, S, base, wbase, width), word) in enumerate(rows):
        assert host(h, pp, n, S, base, wbase, width, C.byref(st)) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
        d = None if pp is None else C.c_void_p(pts.ctypes.data)
        assert dev(h, d, n, S, base, wbase, width, None, C.byref(st)) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    assert st.walk_steps == 5
    # touching ranges do not overlap, and both may end at 2^28 exactly: then the host form's scan finds the bad point and names it
    for base, wbase in ((9, 13), (45, 13), (T - 4, T - 36)):
        assert host(handle, p, 4, 8, base, wbase, 16, C.byref(st)) == WOST_ERR_INVALID and b"point 2 " in lib.wost_last_error(), lib.wost_last_error()
    pts[1, 0] = np.inf
    assert host(handle, p, 4, 8, 0, 4, 16, C.byref(st)) == WOST_ERR_INVALID and b"point 1 " in lib.wost_last_error(), lib.wost_last_error()
    assert st.walk_steps == 5


@pytest.mark.parametrize("pre", PREFIXES)
def test_an_empty_walk_is_ok(pre):
    """n == 0 releases the list; a handle that has none has nothing to release, and no device is asked for"""
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    st = capi.Stats()
    st.walk_steps = 5
    assert getattr(lib, pre + "exits_walk_gradient")(handle, None, 0, 8, 0, 0, 16, C.byref(st)) == 0 and st.walk_steps == 0
    assert getattr(lib, pre + "exits_walk_gradient_dev")(handle, None, 0, 2, 1 << 28, 1 << 28, 16, None, None) == 0
    assert getattr(lib, pre + "exits_walk_gradient")(handle, None, 0, 1, 0, 0, 16, None) == WOST_ERR_INVALID      # (walks < 2 comes first)
    n, S = C.c_int32(-5), C.c_int32(-5)
    assert getattr(lib, pre + "exits_progress")(handle, C.byref(n), C.byref(S)) == 0 and (n.value, S.value) == (0, 0)


@pytest.mark.parametrize("pre", PREFIXES)
def test_apply_and_adjoint_refuse_null_arrays_a_bad_k_and_a_handle_without_a_list(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    colors, grad, se, field = (np.full(54, -1.0, np.float32) for _ in range(4))
    c, g_, s, f = capi._fp(colors), capi._fp(grad), capi._fp(se), capi._fp(field)
    dc, dg, ds, df = (C.c_void_p(a.ctypes.data) for a in (colors, grad, se, field))
    g = lambda name: getattr(lib, pre + "exits_" + name)
    rec = capi.ExitGradientRecords(*[grad.ctypes.data] * 3)
    # every row breaks the rule it names and the rules after it (K = 0, and the zeroed handle holds no list)
    calls = [
        (lambda: g("apply_gradient")(None, c, 0, g_, s, f), b"null"),
        (lambda: g("apply_gradient")(handle, None, 0, g_, s, f), b"null argument: colors"),
        (lambda: g("apply_gradient")(handle, c, 0, None, s, f), b"null argument: grad"),
        (lambda: g("apply_gradient")(handle, c, 0, g_, s, f), b"K must be at least 1"),
        (lambda: g("apply_gradient")(handle, c, -2, g_, None, None), b"K must be at least 1"),
        (lambda: g("apply_gradient")(handle, c, 3, g_, None, None), b"no exit list is bound"),
        (lambda: g("apply_gradient_dev")(None, dc, 0, dg, ds, df, None), b"null"),
        (lambda: g("apply_gradient_dev")(handle, None, 0, dg, ds, df, None), b"null argument: colors"),
        (lambda: g("apply_gradient_dev")(handle, dc, 0, None, ds, df, None), b"null argument: grad"),
        (lambda: g("apply_gradient_dev")(handle, dc, 0, dg, None, None, None), b"K must be at least 1"),
        (lambda: g("apply_gradient_dev")(handle, dc, 1, dg, None, None, None), b"no exit list is bound"),
        (lambda: g("adjoint_gradient")(None, g_, 0, c), b"null"),
        (lambda: g("adjoint_gradient")(handle, None, 0, c), b"null argument: dgrad"),
        (lambda: g("adjoint_gradient")(handle, g_, 0, None), b"null argument: dcolors"),
        (lambda: g("adjoint_gradient")(handle, g_, 0, c), b"K must be at least 1"),
        (lambda: g("adjoint_gradient")(handle, g_, 2, c), b"no exit list is bound"),
        (lambda: g("adjoint_gradient_dev")(None, dg, 0, dc, None), b"null"),
        (lambda: g("adjoint_gradient_dev")(handle, None, 0, dc, None), b"null argument: dgrad"),
        (lambda: g("adjoint_gradient_dev")(handle, dg, 0, None, None), b"null argument: dcolors"),
        (lambda: g("adjoint_gradient_dev")(handle, dg, 0, dc, None), b"K must be at least 1"),
        (lambda: g("adjoint_gradient_dev")(handle, dg, 1, dc, None), b"no exit list is bound"),
        (lambda: g("gradient_records")(None, C.byref(rec)), b"null"),
        (lambda: g("gradient_records")(handle, None), b"null"),
        (lambda: g("gradient_records")(handle, C.byref(rec)), b"no exit list is bound"),
    ]
    for k, (call, word) in enumerate(calls):
        assert call() == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    assert all(np.all(a == -1.0) for a in (colors, grad, se, field))
