"""The continued frame solves of the C-ABI (wost_solve_more, wost_solve_more_sharded, wost_solve_restart, wost_solve_progress
and their wost3_ forms) without a GPU: they exist, include/wost.h declares them, Python knows their prototypes, and an
argument that can be refused before any device work is refused with WOST_ERR_INVALID and a message."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FORMS = ("solve_more", "solve_more_sharded", "solve_restart", "solve_progress")
N_ARGS = {"solve_more": 4, "solve_more_sharded": 7, "solve_restart": 1, "solve_progress": 2}
NAMES = [pre + f for pre in ("wost_", "wost3_") for f in FORMS]
WOST_ERR_INVALID = -1


@pytest.mark.parametrize("name", NAMES)
def test_continued_solves_are_exported_declared_and_prototyped(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == N_ARGS[name.split("_", 1)[1]]
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    assert re.search(r"^int %s\(wost3?_handle h[,)]" % name, header, re.M), name


def _fake_handle():
    """a block of zeroed memory: a call that is refused before the handle is looked at never reads it"""
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


@pytest.mark.parametrize("pre", ["wost_", "wost3_"])
def test_a_null_handle_is_refused(pre):
    from elaina_amd import capi
    lib = capi.load()
    field = np.full(12, -1.0, np.float32)
    n = C.c_int32(7)
    assert getattr(lib, pre + "solve_more")(None, 1, capi._fp(field), None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert getattr(lib, pre + "solve_more_sharded")(None, 0, 1, 1, C.c_void_p(field.ctypes.data), None, None) == WOST_ERR_INVALID
    assert b"null" in lib.wost_last_error()
    assert getattr(lib, pre + "solve_restart")(None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert getattr(lib, pre + "solve_progress")(None, C.byref(n)) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    _keep, handle = _fake_handle()
    assert getattr(lib, pre + "solve_progress")(handle, None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert n.value == 7 and np.all(field == -1.0)


@pytest.mark.parametrize("pre", ["wost_", "wost3_"])
def test_sample_counts_fields_and_shards_are_checked_before_the_handle_is_read(pre):
    """Every refusal below is decided before the handle is looked at or a device is asked for, so it is the same with no GPU
    in the machine."""
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    field = np.full(12, -1.0, np.float32)
    host, dev = capi._fp(field), C.c_void_p(field.ctypes.data)
    more, sharded = getattr(lib, pre + "solve_more"), getattr(lib, pre + "solve_more_sharded")
    st = capi.Stats()
    st.walk_steps = 7
    for bad in (0, -1, 1 << 20):
        assert more(handle, bad, host, C.byref(st)) == WOST_ERR_INVALID
        assert b"more_spp" in lib.wost_last_error() and b"2^20-1" in lib.wost_last_error()
        assert sharded(handle, 0, 1, bad, dev, None, C.byref(st)) == WOST_ERR_INVALID
        assert b"more_spp" in lib.wost_last_error() and b"2^20-1" in lib.wost_last_error()
    assert more(handle, 4, None, None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert sharded(handle, 0, 1, 4, None, None, None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    for index, count in ((0, 0), (0, -2), (-1, 2), (2, 2), (5, 3)):
        assert sharded(handle, index, count, 4, dev, None, None) == WOST_ERR_INVALID and b"shard" in lib.wost_last_error()
    assert np.all(field == -1.0) and st.walk_steps == 7
