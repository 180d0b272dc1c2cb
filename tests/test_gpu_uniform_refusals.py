"""The refusals of the uniform frame solves (wost_solve, wost_solve_sharded and their wost3_ forms) and of the source grid at
create, through ctypes on 8 x 8 handles: every case is an argument the library rejects before any launch, with its code and
message, and the caller's field is left as it was."""
import ctypes as C

import numpy as np
import pytest

from conftest import box_problem, cube_scene3

pytestmark = pytest.mark.gpu

WOST_OK, WOST_ERR_INVALID = 0, -1
SENTINEL = 0x5A
W = H = 8
N_PIXELS = W * H


class _Dim:
    def __init__(self, dim):
        from elaina_amd import UniformIntegrator, UniformIntegratorSettings, capi
        from elaina_amd.integrator3d import Problem3, UniformIntegrator3
        self.dim, self.pre, self.lib = dim, "wost_" if dim == 2 else "wost3_", capi.load()
        st = UniformIntegratorSettings((W, H), 1, 4, 1e-3)
        self.problem = box_problem() if dim == 2 else Problem3.from_dict(cube_scene3(n=1))
        self.it = (UniformIntegrator if dim == 2 else UniformIntegrator3)(self.problem, st)

    def fn(self, name):
        return getattr(self.lib, self.pre + name)

    def error(self):
        return self.lib.wost_last_error().decode()


@pytest.fixture(scope="module", params=[2, 3], ids=["2d", "3d"])
def dim(request):
    d = _Dim(request.param)
    yield d
    d.it.close()


def _host_field():
    return np.frombuffer(bytes([SENTINEL]) * (N_PIXELS * 3 * 4), dtype=np.float32).copy()


def _untouched(a):
    return bool(np.all(a.view(np.uint8) == SENTINEL))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _stale_stats():
    from elaina_amd import capi
    st = capi.Stats()
    st.walk_steps, st.walks_started, st.kernel_launches, st.solve_ms, st.kernel_ms = 7, 5, 3, 1.5, 0.5
    return st


@pytest.mark.parametrize("begin,end", [(-1, N_PIXELS), (0, N_PIXELS + 1), (9, 8)], ids=["begin", "end", "reversed"])
def test_solve_refuses_a_pixel_range_outside_the_frame(dim, begin, end):
    field, st = _host_field(), _stale_stats()
    assert dim.fn("solve")(dim.it._handle, begin, end, _fp(field), C.byref(st)) == WOST_ERR_INVALID
    assert dim.error() == "pixel range outside the frame"
    assert _untouched(field)
    assert st.walk_steps == 7 and st.kernel_launches == 3


@pytest.mark.parametrize("k", [0, 17, N_PIXELS])
def test_solve_of_an_empty_range_is_ok_with_zeroed_stats(dim, k):
    field, st = _host_field(), _stale_stats()
    assert dim.fn("solve")(dim.it._handle, k, k, _fp(field), C.byref(st)) == WOST_OK
    assert all(v == 0 for v in st.as_dict().values())
    assert _untouched(field)
    assert dim.fn("solve")(dim.it._handle, k, k, _fp(field), None) == WOST_OK


def test_solve_refuses_a_null_argument(dim):
    field = _host_field()
    assert dim.fn("solve")(None, 0, N_PIXELS, _fp(field), None) == WOST_ERR_INVALID and dim.error() == "null argument"
    assert dim.fn("solve")(dim.it._handle, 0, N_PIXELS, None, None) == WOST_ERR_INVALID and dim.error() == "null argument"
    assert _untouched(field)


@pytest.mark.parametrize("index,count", [(0, 0), (-1, 2), (2, 2)], ids=["count-0", "index-negative", "index-count"])
def test_solve_sharded_refuses_a_bad_shard(dim, index, count):
    import torch
    field = torch.full((N_PIXELS * 3 * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = _stale_stats()
    assert dim.fn("solve_sharded")(dim.it._handle, index, count, C.c_void_p(field.data_ptr()), None, C.byref(st)) == WOST_ERR_INVALID
    assert dim.error() == "bad shard"
    torch.cuda.synchronize()
    assert bool((field == SENTINEL).all())
    assert st.walk_steps == 7 and st.kernel_launches == 3


def test_solve_sharded_refuses_a_null_field(dim):
    assert dim.fn("solve_sharded")(dim.it._handle, 0, 1, None, None, None) == WOST_ERR_INVALID
    assert dim.error() == "null argument"
    # (the null check comes first)
    assert dim.fn("solve_sharded")(dim.it._handle, 0, 0, None, None, None) == WOST_ERR_INVALID
    assert dim.error() == "null argument"


def test_set_option_refuses_long_steps_beyond_the_order_by_estimate():
    """long_steps is the threshold hand_over reads off the order by estimate, whose key saturates at 32760 (wost_order.h): the
    option takes the multiples of 8 up to there and refuses 32768 and 65528, which it once took.  A refusal leaves the handle's
    setting as it was -- seen in what the next solve sends beside its rounds: with long_steps 8 some of the pixels a persistent
    launch hands over, with 0 (or any value no estimate of this frame reaches) none."""
    from elaina_amd import UniformIntegrator, UniformIntegratorSettings, capi
    it = UniformIntegrator(box_problem(), UniformIntegratorSettings((32, 32), 8, 16, 1e-3))
    lib = capi.load()
    for k, v in {"persist": 1, "resident_blocks": 1, "block_size": 64}.items():
        it.set_option(k, v)

    def beside():
        it.solve()
        ll = it.last_launches()
        assert ll[0]["kind"] == capi.LAUNCH_PERSISTENT and len(ll) >= 2
        return ll[1]["walkers_beside"], any(l["kind"] == capi.LAUNCH_WAIT for l in ll)

    def refused(value):
        assert lib.wost_set_option(it._handle, b"long_steps", float(value)) == WOST_ERR_INVALID
        assert lib.wost_last_error().decode() == "long_steps must be a multiple of 8 in 0..32760 (0 = no pixel runs beside the rounds)"

    assert lib.wost_set_option(it._handle, b"long_steps", 32760.0) == WOST_OK
    assert beside() == (0, False)
    assert lib.wost_set_option(it._handle, b"long_steps", 8.0) == WOST_OK
    for value in (32768, 65528, 32764, -8):
        refused(value)
    n, waited = beside()
    assert n > 0 and waited
    assert lib.wost_set_option(it._handle, b"long_steps", 0.0) == WOST_OK
    for value in (32768, 65528):
        refused(value)
    assert beside() == (0, False)
    it.close()


def test_create_refuses_a_source_grid_without_samples(dim):
    """2-D: a grid with both sizes positive needs its samples.  3-D: a grid with nx > 0 needs the other two sizes and its samples."""
    from elaina_amd import capi
    from elaina_amd.integrator import scene_desc
    from elaina_amd.integrator3d import scene3_desc
    keep = []
    sc = (scene_desc if dim.dim == 2 else scene3_desc)(keep, dim.problem, W, H)
    st = capi.Settings(W, H, 1, 4, 1e-3)
    rgb = np.zeros((2, 2, 2, 3), np.float32)
    sc.source.nx = sc.source.ny = 2
    if dim.dim == 2:
        cases = [(None, None, "source grid without data")]
    else:
        cases = [(0, _fp(rgb), "source grid: bad size or null samples"), (2, None, "source grid: bad size or null samples")]
    for nz, samples, text in cases:
        if dim.dim == 3:
            sc.source.nz = nz
        sc.source.rgb = samples
        out = C.c_void_p(0xDEAD0)
        assert dim.fn("create")(C.byref(sc), C.byref(st), 0, C.byref(out)) == WOST_ERR_INVALID
        assert dim.error() == text
        assert out.value is None
