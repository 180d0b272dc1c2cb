"""The selections, the per-pixel state and the adaptive solves of the carried frame solve in the C-ABI (wost_solve_more_where,
wost_solve_more_where_sharded, wost_solve_carried, wost_solve_adaptive, wost_solve_adaptive_sharded beside wost_solve_progress,
and their wost3_ forms) without a GPU: they exist, include/wost.h declares them, Python knows their prototypes, and an argument
that can be refused before any device work is refused with WOST_ERR_INVALID and a message, the output buffers untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_ARGS = {"solve_more_where": 5, "solve_more_where_sharded": 8, "solve_carried": 5, "solve_adaptive": 6, "solve_adaptive_sharded": 7,
          "solve_progress": 2}
NAMES = [pre + f for pre in ("wost_", "wost3_") for f in N_ARGS]
WOST_ERR_INVALID = -1


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_are_exported_declared_and_prototyped(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == N_ARGS[name.split("_", 1)[1]]
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    assert re.search(r"^int %s\(wost3?_handle h[,)]" % name, header, re.M), name


def test_the_settings_struct_matches_the_header():
    from elaina_amd import capi
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    m = re.search(r"typedef struct wost_adaptive \{(.*?)\} wost_adaptive;", header, re.S)
    assert m
    names = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert names == [n for n, _ in capi.Adaptive._fields_] == ["batch_spp", "min_batches", "max_spp", "abs_tol", "rel_tol"]
    assert C.sizeof(capi.Adaptive) == 20
    # the header no longer speaks of the 20 bytes a pixel carried before it had counts and batch statistics of its own
    assert "52 bytes per" in header and "(20 bytes per pixel" not in header


def _fake_handle():
    """a block of zeroed memory: a call that is refused before the handle is looked at never reads it"""
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


class _Buffers:
    def __init__(self):
        from elaina_amd import capi
        self.field = np.full(12, -1.0, np.float32)
        self.se = np.full(12, -2.0, np.float32)
        self.spp = np.full(4, -3, np.int32)
        self.select = np.ones(4, np.uint8)
        self.stats = capi.Stats()
        self.stats.walk_steps = 7
        self.host, self.dev = capi._fp(self.field), C.c_void_p(self.field.ctypes.data)

    def untouched(self):
        return np.all(self.field == -1.0) and np.all(self.se == -2.0) and np.all(self.spp == -3) and self.stats.walk_steps == 7


@pytest.mark.parametrize("pre", ["wost_", "wost3_"])
def test_null_pointers_are_refused(pre):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    a = capi.Adaptive(4, 4, 64, 0.1, 0.0)
    _keep, handle = _fake_handle()
    sel = b.select.ctypes.data_as(C.POINTER(C.c_uint8))
    calls = [
        lambda: getattr(lib, pre + "solve_more_where")(None, 1, sel, b.host, C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_more_where")(handle, 1, sel, None, C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_more_where_sharded")(None, 0, 1, 1, None, b.dev, None, C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_more_where_sharded")(handle, 0, 1, 1, None, None, None, C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_carried")(None, capi._ip(b.spp), capi._ip(b.spp), b.host, capi._fp(b.se)),
        lambda: getattr(lib, pre + "solve_adaptive")(None, C.byref(a), b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_adaptive")(handle, None, b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_adaptive")(handle, C.byref(a), None, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_adaptive_sharded")(None, 0, 1, C.byref(a), b.dev, None, C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_adaptive_sharded")(handle, 0, 1, None, b.dev, None, C.byref(b.stats)),
        lambda: getattr(lib, pre + "solve_adaptive_sharded")(handle, 0, 1, C.byref(a), None, None, C.byref(b.stats)),
    ]
    for k, call in enumerate(calls):
        assert call() == WOST_ERR_INVALID and b"null" in lib.wost_last_error(), k
    assert b.untouched()


@pytest.mark.parametrize("pre", ["wost_", "wost3_"])
def test_sample_counts_and_shards_of_a_selection_are_checked_before_the_handle_is_read(pre):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    _keep, handle = _fake_handle()
    sel = b.select.ctypes.data_as(C.POINTER(C.c_uint8))
    where, sharded = getattr(lib, pre + "solve_more_where"), getattr(lib, pre + "solve_more_where_sharded")
    for bad in (0, -1, 1 << 20):
        assert where(handle, bad, sel, b.host, C.byref(b.stats)) == WOST_ERR_INVALID
        assert b"more_spp" in lib.wost_last_error() and b"2^20-1" in lib.wost_last_error()
        assert sharded(handle, 0, 1, bad, None, b.dev, None, C.byref(b.stats)) == WOST_ERR_INVALID
        assert b"more_spp" in lib.wost_last_error() and b"2^20-1" in lib.wost_last_error()
    for index, count in ((0, 0), (0, -2), (-1, 2), (2, 2), (5, 3)):
        assert sharded(handle, index, count, 4, None, b.dev, None, C.byref(b.stats)) == WOST_ERR_INVALID and b"shard" in lib.wost_last_error()
    assert b.untouched()


BAD_SETTINGS = [
    ((0, 4, 64, 0.1, 0.0), b"batch_spp"), ((-3, 4, 64, 0.1, 0.0), b"batch_spp"), ((1 << 20, 4, 1 << 21, 0.1, 0.0), b"batch_spp"),
    ((4, 1, 64, 0.1, 0.0), b"min_batches"), ((4, 0, 64, 0.1, 0.0), b"min_batches"), ((4, -2, 64, 0.1, 0.0), b"min_batches"),
    ((4, 4, 3, 0.1, 0.0), b"max_spp"), ((4, 4, 0, 0.1, 0.0), b"max_spp"), ((4, 4, -8, 0.1, 0.0), b"max_spp"),
    ((4, 4, 64, -0.1, 0.0), b"tol"), ((4, 4, 64, 0.1, -1e-9), b"tol"), ((4, 4, 64, float("nan"), 0.0), b"tol"),
    ((4, 4, 64, 0.1, float("nan")), b"tol"), ((4, 4, 64, float("inf"), 0.0), b"tol"), ((4, 4, 64, 0.0, float("inf")), b"tol"),
    ((4, 4, 64, float("-inf"), 0.0), b"tol"),
]


@pytest.mark.parametrize("pre", ["wost_", "wost3_"])
@pytest.mark.parametrize("settings,word", BAD_SETTINGS, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else None)
def test_adaptive_settings_are_checked_before_the_handle_is_read(pre, settings, word):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    _keep, handle = _fake_handle()
    a = capi.Adaptive(*settings)
    assert getattr(lib, pre + "solve_adaptive")(handle, C.byref(a), b.host, capi._fp(b.se), capi._ip(b.spp), C.byref(b.stats)) == WOST_ERR_INVALID
    assert word in lib.wost_last_error(), lib.wost_last_error()
    assert getattr(lib, pre + "solve_adaptive_sharded")(handle, 0, 1, C.byref(a), b.dev, None, C.byref(b.stats)) == WOST_ERR_INVALID
    assert word in lib.wost_last_error(), lib.wost_last_error()
    assert b.untouched()


@pytest.mark.parametrize("pre", ["wost_", "wost3_"])
def test_a_bad_shard_of_an_adaptive_solve_is_refused(pre):
    from elaina_amd import capi
    lib = capi.load()
    b = _Buffers()
    _keep, handle = _fake_handle()
    a = capi.Adaptive(4, 4, 64, 0.1, 0.0)
    for index, count in ((0, 0), (0, -2), (-1, 2), (2, 2), (5, 3)):
        assert getattr(lib, pre + "solve_adaptive_sharded")(handle, index, count, C.byref(a), b.dev, None, C.byref(b.stats)) == WOST_ERR_INVALID
        assert b"shard" in lib.wost_last_error()
    assert b.untouched()
