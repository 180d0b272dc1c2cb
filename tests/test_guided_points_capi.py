"""The guided point solves of the C-ABI (wost_guided_solve_points, wost_guided_solve_points_dev, wost3_guided_solve_points,
wost3_guided_solve_points_dev) without a GPU: they exist, Python knows their prototypes, and an argument that can be refused
before any device work is refused with WOST_ERR_INVALID and a message -- in the order and wording of wost_solve_points
(tests/test_points_capi.py), plus the training override."""
import ctypes as C

import numpy as np
import pytest

POINT_SOLVES = ("wost_guided_solve_points", "wost_guided_solve_points_dev", "wost3_guided_solve_points", "wost3_guided_solve_points_dev")
WOST_ERR_INVALID = -1


def _pointers(capi, name, pts, field):
    dev = name.endswith("_dev")
    return (C.c_void_p(pts.ctypes.data) if dev else capi._fp(pts)), (C.c_void_p(field.ctypes.data) if dev else capi._fp(field))


@pytest.mark.parametrize("name", POINT_SOLVES)
def test_guided_point_solves_are_exported_with_prototypes(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == 8


@pytest.mark.parametrize("name", POINT_SOLVES)
def test_guided_point_solves_refuse_a_null_handle(name):
    from elaina_amd import capi
    lib = capi.load()
    pts = np.zeros(6, np.float32)
    field = np.zeros(6, np.float32)
    p, f = _pointers(capi, name, pts, field)
    assert getattr(lib, name)(None, p, 2, 0, 16, -1, f, None) == WOST_ERR_INVALID
    assert len(lib.wost_last_error()) > 0
    assert b"null" in lib.wost_last_error()
    assert not field.any()


@pytest.mark.parametrize("name", POINT_SOLVES)
def test_guided_point_solves_check_their_arguments_before_any_device_work(name):
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
    p, f = _pointers(capi, name, pts, field)

    def call(n, seed_base, seed_width, train_spp=-1, pp=p, ff=f, st=None):
        return getattr(lib, name)(handle, pp, n, seed_base, seed_width, train_spp, ff, st)

    assert call(4, 0, 16, pp=None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert call(4, 0, 16, ff=None) == WOST_ERR_INVALID and b"null" in lib.wost_last_error()
    assert call(-1, 0, 16) == WOST_ERR_INVALID and b"negative" in lib.wost_last_error()
    assert call(4, 0, 0) == WOST_ERR_INVALID and b"seed_width" in lib.wost_last_error()
    assert call(4, 0, -3) == WOST_ERR_INVALID and b"seed_width" in lib.wost_last_error()
    assert call(4, -1, 16) == WOST_ERR_INVALID and b"seed_base" in lib.wost_last_error()
    assert call(4, (1 << 28) - 3, 16) == WOST_ERR_INVALID and b"2^28" in lib.wost_last_error()
    assert call(4, 0, 16, train_spp=-2) == WOST_ERR_INVALID and b"train_spp_count" in lib.wost_last_error()
    # the order of wost_solve_points: the list's length before the seeds, the seeds before the training override
    assert call(-1, -1, 0, train_spp=-2) == WOST_ERR_INVALID and b"negative" in lib.wost_last_error()
    assert call(4, -1, 16, train_spp=-2) == WOST_ERR_INVALID and b"seed_base" in lib.wost_last_error()
    assert call(0, 1 << 28, 16) == 0                     # the seed range may end at 2^28
    assert call(0, 0, 16, train_spp=0) == 0 and call(0, 0, 16, train_spp=7) == 0
    st = capi.GuidedStats()
    st.walk_steps, st.kernel_launches, st.train_samples, st.solve_ms = 7, 3, 5, 2.0
    assert call(0, 0, 16, st=C.byref(st)) == 0
    assert st.walk_steps == 0 and st.kernel_launches == 0 and st.train_samples == 0 and st.solve_ms == 0.0
    if not dev:
        # the host variants scan the list: the first bad index is named
        pts[2 * dim + 1] = np.inf
        assert call(4, 0, 16) == WOST_ERR_INVALID and b"point 2 " in lib.wost_last_error()
        pts[1 * dim] = np.nan
        assert call(4, 0, 16) == WOST_ERR_INVALID and b"point 1 " in lib.wost_last_error()
    assert np.all(field == -1.0)
