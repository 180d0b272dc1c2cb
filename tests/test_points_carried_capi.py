"""The carried point list in the C-ABI (wost_points_carry, _carry_dev, _more, _more_dev, _carried, _adaptive, _adaptive_dev,
_restart, _progress and their wost3_ forms) without a GPU: the eighteen names exist, include/wost.h declares them, Python knows
their prototypes, and every argument that can be refused before any device work is refused with WOST_ERR_INVALID and a message,
the output buffers untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_adaptive_capi import BAD_SETTINGS, _Buffers, _fake_handle

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_ARGS = {"points_carry": 5, "points_carry_dev": 6, "points_more": 5, "points_more_dev": 6, "points_carried": 5, "points_adaptive": 6,
          "points_adaptive_dev": 5, "points_restart": 1, "points_progress": 3}
NAMES = [pre + f for pre in ("wost_", "wost3_") for f in N_ARGS]
PREFIXES = ["wost_", "wost3_"]
WOST_ERR_INVALID = -1


def test_there_are_eighteen_names():
    assert len(NAMES) == len(set(NAMES)) == 18


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


def test_the_header_no_longer_says_that_point_lists_are_not_carried():
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    for m in re.finditer(r"Not carried:[^*]*\*/|Not carried:[^.]*\.", header, re.S):
        assert "point lists" not in m.group(0), m.group(0)
    assert "point lists" not in header
    assert "The carried point list" in header


def test_the_library_version_was_raised():
    from elaina_amd import capi
    assert b"0.3" in capi.load().wost_version()


def _pts(pre, n=4):
    return np.zeros((n, 2 if pre == "wost_" else 3), np.float32)


@pytest.mark.parametrize("pre", PREFIXES)
def test_a_bind_is_checked_in_the_documented_order_before_the_handle_is_read(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    pts = _pts(pre)
    p = capi._fp(pts)
    host, dev = getattr(lib, pre + "points_carry"), getattr(lib, pre + "points_carry_dev")
    # (arguments after the handle: points, n, seed_base, seed_width) -> the word of the refusal; every row breaks the rule it
    # names and every rule after it, so the order shows
    rows = [
        ((None, p, -1, -1, 0), b"null"),
        ((handle, None, -1, -1, 0), b"negative"),
        ((handle, None, 4, -1, 0), b"null"),
        ((handle, p, 4, -1, 0), b"seed_width"),
        ((handle, p, 4, -1, -16), b"seed_width"),
        ((handle, p, 4, -1, 16), b"seed_base"),
        ((handle, p, 4, (1 << 28) - 3, 16), b"2^28"),
    ]
    for k, ((h, pp, n, base, width), word) in enumerate(rows):
        assert host(h, pp, n, base, width) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
        d = None if pp is None else C.c_void_p(pts.ctypes.data)
        assert dev(h, d, n, base, width, None) == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())


@pytest.mark.parametrize("pre", PREFIXES)
def test_a_host_bind_names_the_first_point_that_is_not_finite(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    pts = _pts(pre, 9)
    pts[7, 0] = np.inf
    pts[5, -1] = np.nan
    assert getattr(lib, pre + "points_carry")(handle, capi._fp(pts), 9, 0, 16) == WOST_ERR_INVALID
    assert b"point 5 " in lib.wost_last_error(), lib.wost_last_error()


@pytest.mark.parametrize("pre", PREFIXES)
def test_null_pointers_are_refused(pre):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    a = capi.Adaptive(4, 4, 64, 0.1, 0.0)
    _keep, handle = _fake_handle()
    sel = b.select.ctypes.data_as(C.POINTER(C.c_uint8))
    n = C.c_int32(-5)
    f = lambda name: getattr(lib, pre + name)
    calls = [
        lambda: f("points_more")(None, 1, sel, b.host, C.byref(b.stats)),
        lambda: f("points_more")(handle, 1, sel, None, C.byref(b.stats)),
        lambda: f("points_more_dev")(None, 1, None, b.dev, None, C.byref(b.stats)),
        lambda: f("points_more_dev")(handle, 1, None, None, None, C.byref(b.stats)),
        lambda: f("points_carried")(None, capi._ip(b.spp), capi._ip(b.spp), b.host, capi._fp(b.se)),
        lambda: f("points_adaptive")(None, C.byref(a), b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: f("points_adaptive")(handle, None, b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: f("points_adaptive")(handle, C.byref(a), None, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: f("points_adaptive_dev")(None, C.byref(a), b.dev, None, C.byref(b.stats)),
        lambda: f("points_adaptive_dev")(handle, None, b.dev, None, C.byref(b.stats)),
        lambda: f("points_adaptive_dev")(handle, C.byref(a), None, None, C.byref(b.stats)),
        lambda: f("points_restart")(None),
        lambda: f("points_progress")(None, C.byref(n), C.byref(n)),
        lambda: f("points_progress")(handle, None, C.byref(n)),
        lambda: f("points_progress")(handle, C.byref(n), None),
    ]
    for k, call in enumerate(calls):
        assert call() == WOST_ERR_INVALID and b"null" in lib.wost_last_error(), k
    assert b.untouched() and n.value == -5


@pytest.mark.parametrize("pre", PREFIXES)
def test_sample_counts_are_checked_before_the_handle_is_read(pre):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    _keep, handle = _fake_handle()
    sel = b.select.ctypes.data_as(C.POINTER(C.c_uint8))
    for bad in (0, -1, 1 << 20):
        assert getattr(lib, pre + "points_more")(handle, bad, sel, b.host, C.byref(b.stats)) == WOST_ERR_INVALID
        assert b"more_spp" in lib.wost_last_error() and b"2^20-1" in lib.wost_last_error()
        assert getattr(lib, pre + "points_more_dev")(handle, bad, None, b.dev, None, C.byref(b.stats)) == WOST_ERR_INVALID
        assert b"more_spp" in lib.wost_last_error() and b"2^20-1" in lib.wost_last_error()
    assert b.untouched()


@pytest.mark.parametrize("pre", PREFIXES)
@pytest.mark.parametrize("settings,word", BAD_SETTINGS, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else None)
def test_adaptive_settings_are_refused_in_the_words_of_the_frame_solve(pre, settings, word):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    _keep, handle = _fake_handle()
    a = capi.Adaptive(*settings)
    frame = pre + "solve_adaptive"
    assert getattr(lib, frame)(handle, C.byref(a), b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)) == WOST_ERR_INVALID
    words = lib.wost_last_error()
    assert word in words
    assert getattr(lib, pre + "points_adaptive")(handle, C.byref(a), b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)) == WOST_ERR_INVALID
    assert lib.wost_last_error() == words
    assert getattr(lib, pre + "points_adaptive_dev")(handle, C.byref(a), b.dev, None, C.byref(b.stats)) == WOST_ERR_INVALID
    assert lib.wost_last_error() == words
    assert b.untouched()


@pytest.mark.parametrize("pre", PREFIXES)
def test_calls_without_a_bound_list_say_so(pre):
    """a zeroed handle has no list: the calls that need one are refused once their own arguments have passed"""
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    a = capi.Adaptive(4, 4, 64, 0.1, 0.0)
    _keep, handle = _fake_handle()
    f = lambda name: getattr(lib, pre + name)
    calls = [
        lambda: f("points_more")(handle, 3, None, b.host, C.byref(b.stats)),
        lambda: f("points_more_dev")(handle, 3, None, b.dev, None, C.byref(b.stats)),
        lambda: f("points_carried")(handle, capi._ip(b.spp), capi._ip(b.spp), b.host, capi._fp(b.se)),
        lambda: f("points_adaptive")(handle, C.byref(a), b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: f("points_adaptive_dev")(handle, C.byref(a), b.dev, None, C.byref(b.stats)),
    ]
    for k, call in enumerate(calls):
        assert call() == WOST_ERR_INVALID and b"no point list is bound" in lib.wost_last_error(), (k, lib.wost_last_error())
    assert b.untouched()
    # progress and restart need no list
    n, done = C.c_int32(-5), C.c_int32(-5)
    assert f("points_progress")(handle, C.byref(n), C.byref(done)) == 0 and (n.value, done.value) == (0, 0)
    assert f("points_restart")(handle) == 0
