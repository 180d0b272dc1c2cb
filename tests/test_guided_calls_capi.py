"""The entry points that the 2-D and the 3-D guided solve have in common (wost_guided_* and wost3_guided_*: network, scene, solve,
solve_sharded, query_network, train_set, destroy) without a GPU: an argument that can be refused before the handle is looked at
is refused with WOST_ERR_INVALID and the same words on both sides, and the two Python integrators offer the shared methods with
equal signatures.  (The point solves: tests/test_guided_points_capi.py; "bad shard" needs a live handle: tests/test_gpu_guided_calls.py.)"""
import ctypes as C
import inspect

import numpy as np
import pytest

PREFIXES = ("wost_guided_", "wost3_guided_")
WOST_OK, WOST_ERR_INVALID = 0, -1
SHARED_METHODS = ("close", "__del__", "solve", "solve_sharded", "solve_points", "solve_points_dev", "train_set", "queryNetwork")


@pytest.fixture(scope="module")
def lib():
    from elaina_amd import capi
    return capi.load()


@pytest.fixture()
def fake():
    """a handle of zeroed memory: no refusal below may read it"""
    buf = C.create_string_buffer(1 << 16)
    yield C.c_void_p(C.addressof(buf))
    assert buf.raw == bytes(1 << 16)


def _refused(lib, rc, words):
    assert rc == WOST_ERR_INVALID, rc
    assert lib.wost_last_error() == words, lib.wost_last_error()


@pytest.mark.parametrize("prefix", PREFIXES)
def test_network_and_scene_refuse_null_arguments(lib, fake, prefix):
    for name in ("network", "scene"):
        fn = getattr(lib, prefix + name)
        out = C.c_void_p(0x1234)
        _refused(lib, fn(None, C.byref(out)), b"null argument")
        _refused(lib, fn(fake, None), b"null argument")
        assert out.value == 0x1234


@pytest.mark.parametrize("prefix", PREFIXES)
def test_solves_refuse_null_arguments(lib, fake, prefix):
    from elaina_amd import capi
    field = np.full(12, -1.0, np.float32)
    st = capi.GuidedStats()
    st.walk_steps = 7
    solve, sharded = getattr(lib, prefix + "solve"), getattr(lib, prefix + "solve_sharded")
    _refused(lib, solve(None, capi._fp(field), C.byref(st)), b"null argument")
    _refused(lib, solve(fake, None, C.byref(st)), b"null argument")
    _refused(lib, sharded(None, 0, 1, C.c_void_p(field.ctypes.data), C.byref(st)), b"null argument")
    _refused(lib, sharded(fake, 0, 1, None, C.byref(st)), b"null argument")
    # the null handle is named before the shard is looked at
    _refused(lib, sharded(None, 3, 2, C.c_void_p(field.ctypes.data), C.byref(st)), b"null argument")
    assert np.all(field == -1.0) and st.walk_steps == 7


@pytest.mark.parametrize("prefix", PREFIXES)
def test_query_network_refuses_null_arguments_and_a_negative_count(lib, fake, prefix):
    from elaina_amd import capi
    fn = getattr(lib, prefix + "query_network")
    pts, raw = np.zeros(12, np.float32), np.full(4 * 41, -1.0, np.float32)
    _refused(lib, fn(None, capi._fp(pts), 4, capi._fp(raw)), b"bad argument")
    _refused(lib, fn(fake, None, 4, capi._fp(raw)), b"bad argument")
    _refused(lib, fn(fake, capi._fp(pts), 4, None), b"bad argument")
    _refused(lib, fn(fake, capi._fp(pts), -1, capi._fp(raw)), b"bad argument")
    assert np.all(raw == -1.0)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_train_set_refuses_null_arguments_and_a_negative_capacity(lib, fake, prefix):
    fn = getattr(lib, prefix + "train_set")
    n = C.c_int32(-5)
    _refused(lib, fn(None, 0, C.byref(n), None, None, None, None, None, None), b"bad argument")
    _refused(lib, fn(fake, 0, None, None, None, None, None, None, None), b"bad argument")
    _refused(lib, fn(fake, -1, C.byref(n), None, None, None, None, None, None), b"bad argument")
    assert n.value == -5


@pytest.mark.parametrize("prefix", PREFIXES)
def test_destroy_of_a_null_handle_is_ok(lib, prefix):
    assert getattr(lib, prefix + "destroy")(None) == WOST_OK


def test_the_two_integrators_share_their_methods_with_equal_signatures():
    from elaina_amd.guided import GuidedIntegrator
    from elaina_amd.integrator3d import GuidedIntegrator3
    for name in SHARED_METHODS:
        a, b = getattr(GuidedIntegrator, name), getattr(GuidedIntegrator3, name)
        assert callable(a) and callable(b), name
        assert inspect.signature(a) == inspect.signature(b), (name, inspect.signature(a), inspect.signature(b))
