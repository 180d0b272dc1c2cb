"""The gradient calls of the C-ABI (wost_solve_gradient_points, wost_solve_gradient_points_dev and their wost3_ twins) without
a GPU: they exist, Python knows their prototypes and the struct of their outputs, and an argument that can be refused before the
handle is read is refused with WOST_ERR_INVALID and a message, with every output untouched."""
import ctypes as C

import numpy as np
import pytest

GRADIENT_CALLS = ("wost_solve_gradient_points", "wost_solve_gradient_points_dev", "wost3_solve_gradient_points",
                  "wost3_solve_gradient_points_dev")
WOST_ERR_INVALID = -1
S_FAKE = 4      # the first points of the calls below are sized for 4 walks per point; no call gets far enough to write them


def test_the_output_struct_is_five_pointers():
    from elaina_amd import capi
    assert [f[0] for f in capi.GradientOut._fields_] == ["grad", "grad_stderr", "field_rgb", "radius", "first_pts"]
    assert C.sizeof(capi.GradientOut) == 5 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("name", GRADIENT_CALLS)
def test_gradient_calls_are_exported_with_prototypes(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == (9 if name.endswith("_dev") else 8)
    assert fn.argtypes[6] == C.POINTER(capi.GradientOut)


@pytest.mark.parametrize("name", GRADIENT_CALLS)
def test_gradient_calls_check_their_arguments_before_the_handle_is_read(name):
    """Every refusal below, and the empty list, is decided before the handle is looked at or a device is asked for, so it is
    the same with no GPU in the machine.  (The handle here is a block of zeroed memory: none of these calls may read it.)"""
    from elaina_amd import capi
    lib = capi.load()
    dev = name.endswith("_dev")
    dim = 3 if name.startswith("wost3") else 2
    fake = C.create_string_buffer(1 << 16)
    handle = C.c_void_p(C.addressof(fake))
    pts = np.zeros(4 * dim, np.float32)
    outs = {"grad": np.full(4 * dim * 3, -1.0, np.float32), "grad_stderr": np.full(4 * dim * 3, -1.0, np.float32),
            "field_rgb": np.full(12, -1.0, np.float32), "radius": np.full(4, -1.0, np.float32),
            "first_pts": np.full(4 * S_FAKE * dim, -1.0, np.float32)}
    go = capi.GradientOut(*[outs[f[0]].ctypes.data for f in capi.GradientOut._fields_])
    p = C.c_void_p(pts.ctypes.data) if dev else capi._fp(pts)

    def call(n, seed_base, walk_seed_base, seed_width, h=handle, pp=p, out=C.byref(go), st=None):
        args = [h, pp, n, seed_base, walk_seed_base, seed_width, out] + ([None] if dev else [])
        return getattr(lib, name)(*args, st)

    def refused(word, *args, **kw):
        assert call(*args, **kw) == WOST_ERR_INVALID
        assert word in lib.wost_last_error(), lib.wost_last_error()

    refused(b"null", 4, 0, 100, 16, h=None)
    refused(b"null", 4, 0, 100, 16, pp=None)
    refused(b"null", 4, 0, 100, 16, out=None)
    no_grad = capi.GradientOut(None, outs["grad_stderr"].ctypes.data, None, None, None)
    refused(b"null", 4, 0, 100, 16, out=C.byref(no_grad))
    refused(b"negative", -1, 0, 100, 16)
    refused(b"seed_width", 4, 0, 100, 0)
    refused(b"seed_width", 4, 0, 100, -3)
    refused(b"seed_base", 4, -1, 100, 16)
    refused(b"seed_base", 4, 0, -1, 16)
    refused(b"2^28", 4, (1 << 28) - 3, 0, 16)
    assert call(0, 1 << 28, 0, 16) == 0                     # the seed range may end at 2^28
    st = capi.Stats()
    st.walk_steps, st.kernel_launches = 7, 3
    assert call(0, 0, 0, 16, st=C.byref(st)) == 0           # (an empty list has no seed ranges to overlap)
    assert st.walk_steps == 0 and st.kernel_launches == 0 and st.solve_ms == 0.0
    if not dev:
        # the host forms scan the list: the first bad point is named
        pts[2 * dim + 1] = np.inf
        refused(b"point 2 ", 4, 0, 100, 16)
        pts[1 * dim] = np.nan
        refused(b"point 1 ", 4, 0, 100, 16)
    for a in outs.values():
        assert np.all(a == -1.0)
