"""The exit list in the C-ABI (wost_exits_walk, _walk_dev, _records, _apply, _apply_dev, _adjoint, _adjoint_dev, _progress and their
wost3_ forms) without a GPU: the sixteen names exist, include/wost.h declares them, Python knows their prototypes and the struct,
and every argument that can be refused before the handle is read is refused with WOST_ERR_INVALID, in the order of the header,
with a message that names the quantity and the outputs untouched.  (The handle is a block of zeroed memory: none of these
refusals may read more of it than the fact that it holds no list.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_ARGS = {"exits_walk": 7, "exits_walk_dev": 8, "exits_records": 2, "exits_apply": 5, "exits_apply_dev": 6, "exits_adjoint": 4,
          "exits_adjoint_dev": 5, "exits_progress": 3}
PREFIXES = ["wost_", "wost3_"]
NAMES = [pre + f for pre in PREFIXES for f in N_ARGS]
WOST_ERR_INVALID = -1


def _fake_handle():
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


def test_there_are_sixteen_names_and_the_struct_has_the_stated_fields():
    from elaina_amd import capi
    assert len(NAMES) == len(set(NAMES)) == 16
    assert [f[0] for f in capi.ExitRecords._fields_] == ["prim", "uv", "side", "thp", "base_rgb"]
    assert C.sizeof(capi.ExitRecords) == 5 * C.sizeof(C.c_void_p)
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    m = re.search(r"typedef struct wost_exit_records \{(.*?)\} wost_exit_records;", header, re.S)
    assert re.findall(r"\*(\w+);", m.group(1)) == ["prim", "uv", "side", "thp", "base_rgb"]


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
    host, dev = getattr(lib, pre + "exits_walk"), getattr(lib, pre + "exits_walk_dev")
    T = 1 << 28
    # (handle, points, n, walks, walk_seed_base, seed_width) -> the word of the refusal; every row breaks the rule it names and,
    # as far as one call can, the rules after it, so the order shows
    rows = [
        ((None, p, -1, 0, -1, 0), b"null"),
        ((handle, None, -1, 0, -1, 0), b"negative"),
        ((handle, None, 4, 0, -1, 0), b"null"),
        ((handle, p, 4, 0, -1, 0), b"walks"),
        ((handle, p, 4, -3, -1, 0), b"walks"),
        ((handle, p, 4, 8, -1, 0), b"seed_width"),
        ((handle, p, 4, 8, -1, -16), b"seed_width"),
        ((handle, p, 4, 8, -1, 16), b"walk_seed_base"),
        # the seeds end at (2^28 - 31) + 4 * 8 = 2^28 + 1
        ((handle, p, 4, 8, T - 31, 16), b"walk_seed_base + n * walks"),
        # ... and in 64 bits: 2^24 points times 256 walks is 2^32, which is 0 in 32 bits
        ((handle, p, 1 << 24, 256, 0, 16), b"walk_seed_base + n * walks"),
    ]
    st = capi.Stats()
    st.walk_steps = 5
    for k, ((h, pp, n, S, base, width), word) in enumerate(rows):
        assert host(h, pp, n, S, base, width, C.byref(st)) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
        d = None if pp is None else C.c_void_p(pts.ctypes.data)
        assert dev(h, d, n, S, base, width, None, C.byref(st)) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    assert b"2^28" in lib.wost_last_error() and st.walk_steps == 5
    # the seeds may end at 2^28 exactly: then the host form's scan finds the bad point and names it
    assert host(handle, p, 4, 8, T - 32, 16, C.byref(st)) == WOST_ERR_INVALID and b"point 2 " in lib.wost_last_error(), lib.wost_last_error()
    pts[1, 0] = np.inf
    assert host(handle, p, 4, 8, 0, 16, C.byref(st)) == WOST_ERR_INVALID and b"point 1 " in lib.wost_last_error(), lib.wost_last_error()
    assert st.walk_steps == 5


@pytest.mark.parametrize("pre", PREFIXES)
def test_an_empty_walk_is_ok(pre):
    """n == 0 releases the list; a handle that has none has nothing to release, and no device is asked for"""
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    st = capi.Stats()
    st.walk_steps = 5
    assert getattr(lib, pre + "exits_walk")(handle, None, 0, 8, 0, 16, C.byref(st)) == 0 and st.walk_steps == 0
    assert getattr(lib, pre + "exits_walk_dev")(handle, None, 0, 1, 1 << 28, 16, None, None) == 0
    n, S = C.c_int32(-5), C.c_int32(-5)
    assert getattr(lib, pre + "exits_progress")(handle, C.byref(n), C.byref(S)) == 0 and (n.value, S.value) == (0, 0)


@pytest.mark.parametrize("pre", PREFIXES)
def test_apply_and_adjoint_refuse_null_arrays_a_bad_k_and_a_handle_without_a_list(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    colors, field, se = (np.full(36, -1.0, np.float32) for _ in range(3))
    c, f, s = capi._fp(colors), capi._fp(field), capi._fp(se)
    dc, df, ds = (C.c_void_p(a.ctypes.data) for a in (colors, field, se))
    g = lambda name: getattr(lib, pre + "exits_" + name)
    n = C.c_int32(-5)
    rec = capi.ExitRecords(*[field.ctypes.data] * 5)
    # every row breaks the rule it names and the rules after it (K = 0, and the zeroed handle holds no list)
    calls = [
        (lambda: g("apply")(None, c, 0, f, s), b"null"),
        (lambda: g("apply")(handle, None, 0, f, s), b"null argument: colors"),
        (lambda: g("apply")(handle, c, 0, None, s), b"null argument: field_rgb"),
        (lambda: g("apply")(handle, c, 0, f, s), b"K must be at least 1"),
        (lambda: g("apply")(handle, c, -2, f, None), b"K must be at least 1"),
        (lambda: g("apply")(handle, c, 3, f, s), b"no exit list is bound"),
        (lambda: g("apply_dev")(None, dc, 0, df, ds, None), b"null"),
        (lambda: g("apply_dev")(handle, None, 0, df, ds, None), b"null argument: colors"),
        (lambda: g("apply_dev")(handle, dc, 0, None, None, None), b"null argument: field_rgb"),
        (lambda: g("apply_dev")(handle, dc, 0, df, None, None), b"K must be at least 1"),
        (lambda: g("apply_dev")(handle, dc, 1, df, None, None), b"no exit list is bound"),
        (lambda: g("adjoint")(None, f, 0, c), b"null"),
        (lambda: g("adjoint")(handle, None, 0, c), b"null argument: dfield"),
        (lambda: g("adjoint")(handle, f, 0, None), b"null argument: dcolors"),
        (lambda: g("adjoint")(handle, f, 0, c), b"K must be at least 1"),
        (lambda: g("adjoint")(handle, f, 2, c), b"no exit list is bound"),
        (lambda: g("adjoint_dev")(None, df, 0, dc, None), b"null"),
        (lambda: g("adjoint_dev")(handle, None, 0, dc, None), b"null argument: dfield"),
        (lambda: g("adjoint_dev")(handle, df, 0, None, None), b"null argument: dcolors"),
        (lambda: g("adjoint_dev")(handle, df, 0, dc, None), b"K must be at least 1"),
        (lambda: g("adjoint_dev")(handle, df, 1, dc, None), b"no exit list is bound"),
        (lambda: g("records")(None, C.byref(rec)), b"null"),
        (lambda: g("records")(handle, None), b"null"),
        (lambda: g("records")(handle, C.byref(rec)), b"no exit list is bound"),
        (lambda: g("progress")(None, C.byref(n), C.byref(n)), b"null"),
        (lambda: g("progress")(handle, None, C.byref(n)), b"null"),
        (lambda: g("progress")(handle, C.byref(n), None), b"null"),
    ]
    for k, (call, word) in enumerate(calls):
        assert call() == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    assert all(np.all(a == -1.0) for a in (colors, field, se)) and n.value == -5
