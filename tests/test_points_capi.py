"""The point solves of the C-ABI (wost_solve_points, wost_solve_points_dev, wost3_solve_points, wost3_solve_points_dev)
without a GPU: they exist, Python knows their prototypes, and an argument that can be refused before any device work is
refused with WOST_ERR_INVALID and a message."""
import ctypes as C

import numpy as np
import pytest

POINT_SOLVES = ("wost_solve_points", "wost_solve_points_dev", "wost3_solve_points", "wost3_solve_points_dev")
WOST_ERR_INVALID = -1


def _call(lib, name, handle, pts, n, seed_base, seed_width, field):
    args = [handle, pts, n, seed_base, seed_width, field]
    if name.endswith("_dev"):
        args.append(None)      # the stream
    return getattr(lib, name)(*args, None)


@pytest.mark.parametrize("name", POINT_SOLVES)
def test_point_solves_are_exported_with_prototypes(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == (8 if name.endswith("_dev") else 7)


@pytest.mark.parametrize("name", POINT_SOLVES)
def test_point_solves_refuse_a_null_handle(name):
    from elaina_amd import capi
    lib = capi.load()
    dev = name.endswith("_dev")
    pts = np.zeros(6, np.float32)
    field = np.zeros(6, np.float32)
    p = C.c_void_p(pts.ctypes.data) if dev else capi._fp(pts)
    f = C.c_void_p(field.ctypes.data) if dev else capi._fp(field)
    assert _call(lib, name, None, p, 2, 0, 16, f) == WOST_ERR_INVALID
    assert len(lib.wost_last_error()) > 0
    assert b"null" in lib.wost_last_error()
    assert not field.any()


@pytest.mark.parametrize("name", POINT_SOLVES)
def test_point_solves_check_their_arguments_before_any_device_work(name):
    """Every refusal below, and the empty list, is decided before the handle is looked at or a device is asked for, so it is
    the same with no GPU in the machine.  (The handle here is a block of zeroed memory: none of these calls may read it.)"""
    from elaina_amd import capi
    lib = capi.load()
    dev = name.endswith("_dev")
    dim = 3 if name.startswith("wost3") else 2
    fake = C.create_string_buffer(1 << 16)
    handle = C.c_void_p(C.addressof(fake))
    pts = np.zeros(4 * dim, np.float32)
    field = np.full(12, -1.0, np.float32)
    p = C.c_void_p(pts.ctypes.data) if dev else capi._fp(pts)
    f = C.c_void_p(field.ctypes.data) if dev else capi._fp(field)

    def call(n, seed_base, seed_width, pp=p, ff=f, st=None):
        args = [handle, pp, n, seed_base, seed_width, ff] + ([None] if dev else [])
        return getattr(lib, name)(*args, st)

    assert call(4, 0, 16, pp=None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert call(4, 0, 16, ff=None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert call(-1, 0, 16) == WOST_ERR_INVALID and b"negative" in lib.wost_last_error()
    assert call(4, 0, 0) == WOST_ERR_INVALID and b"seed_width" in lib.wost_last_error()
    assert call(4, 0, -3) == WOST_ERR_INVALID and b"seed_width" in lib.wost_last_error()
    assert call(4, -1, 16) == WOST_ERR_INVALID and b"seed_base" in lib.wost_last_error()
    assert call(4, (1 << 28) - 3, 16) == WOST_ERR_INVALID and b"2^28" in lib.wost_last_error()
    assert call(0, 1 << 28, 16) == 0                     # the seed range may end at 2^28
    st = capi.Stats()
    st.walk_steps, st.kernel_launches = 7, 3
    assert call(0, 0, 16, st=C.byref(st)) == 0
    assert st.walk_steps == 0 and st.kernel_launches == 0 and st.solve_ms == 0.0
    if not dev:
        # the host variants scan the list: the first bad index is named
        pts[2 * dim + 1] = np.inf
        assert call(4, 0, 16) == WOST_ERR_INVALID and b"point 2 " in lib.wost_last_error()
        pts[1 * dim] = np.nan
        assert call(4, 0, 16) == WOST_ERR_INVALID and b"point 1 " in lib.wost_last_error()
    assert np.all(field == -1.0)
