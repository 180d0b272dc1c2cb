"""The refusals of wost_create and wost3_create that are decided before a device is asked for, so they are the same with no
GPU in the machine: the code, the message, the order of the checks, and a null *out in every refused case.  The two
dimensions differ in one rule on purpose: 2-D packs a walker's sample and depth into 20 and 10 bits and refuses what does not
fit; 3-D has no such limit and goes on to the device check."""
import ctypes as C

import pytest

WOST_OK, WOST_ERR_INVALID, WOST_ERR_DEVICE, WOST_ERR_UNSUPPORTED = 0, -1, -2, -3
STALE = 0xDEAD0       # what *out holds before the call: a refusal past the null checks leaves a null there


def _create(dim, settings=(8, 8, 1, 4), scene=True, with_settings=True, with_out=True, before=STALE):
    """(return code, message, *out) of a create call on an empty scene"""
    from elaina_amd import capi
    lib = capi.load()
    sc = (capi.SceneDesc if dim == 2 else capi.Scene3Desc)()
    st = capi.Settings(*settings, 1e-3)
    out = C.c_void_p(before)
    fn = lib.wost_create if dim == 2 else lib.wost3_create
    rc = fn(C.byref(sc) if scene else None, C.byref(st) if with_settings else None, 0, C.byref(out) if with_out else None)
    return rc, lib.wost_last_error().decode(), out.value, lib


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("missing", ["scene", "settings", "out"])
def test_create_refuses_a_null_argument(dim, missing):
    rc, msg, out, _ = _create(dim, scene=missing != "scene", with_settings=missing != "settings", with_out=missing != "out", before=None)
    assert rc == WOST_ERR_INVALID and msg == "null argument"
    assert out is None


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("settings", [(0, 8, 1, 4), (8, 0, 1, 4), (8, 8, 1, 0), (8, 8, -1, 4)], ids=["width", "height", "max_depth", "spp"])
def test_create_refuses_bad_settings(dim, settings):
    rc, msg, out, _ = _create(dim, settings)
    assert rc == WOST_ERR_INVALID and msg == "bad settings"
    assert out is None


@pytest.mark.parametrize("dim", [2, 3])
def test_create_refuses_a_frame_too_large(dim):
    rc, msg, out, _ = _create(dim, (16385, 16385, 1, 4))
    assert rc == WOST_ERR_UNSUPPORTED and msg == "frame too large"
    assert out is None
    # (2-D tests its packing limits first)
    rc, msg, out, _ = _create(dim, (16385, 16385, 1 << 20, 4))
    assert rc == WOST_ERR_UNSUPPORTED and msg == ("spp must be < 2^20 and max_depth < 2^10" if dim == 2 else "frame too large")
    assert out is None


@pytest.mark.parametrize("settings", [(8, 8, 1 << 20, 4), (8, 8, 1, 1 << 10)], ids=["spp", "max_depth"])
def test_create_2d_refuses_what_a_walker_cannot_pack(settings):
    rc, msg, out, _ = _create(2, settings)
    assert rc == WOST_ERR_UNSUPPORTED and msg == "spp must be < 2^20 and max_depth < 2^10"
    assert out is None


@pytest.mark.parametrize("settings", [(8, 8, 1 << 20, 4), (8, 8, 1, 1 << 10)], ids=["spp", "max_depth"])
def test_create_3d_has_no_packing_limit(settings):
    """the call goes on to the device check: with no GPU that is where it ends, with one it makes the handle"""
    rc, msg, out, lib = _create(3, settings)
    if rc == WOST_OK:
        assert out is not None and out != STALE
        assert lib.wost3_destroy(C.c_void_p(out)) == WOST_OK
    else:
        assert rc == WOST_ERR_DEVICE and msg.startswith("no HIP device")
        assert out is None
