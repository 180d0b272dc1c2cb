"""The in-ball term of the gradient without a GPU: the emulation of gradient_source_emulation.py against closed forms, and the
option door of the C-ABI (wost_set_option "grad_source", wost3_set_option) on a zeroed block of memory in place of a handle.

Closed forms.  For the source f_c = a_c + b_c x_1 (bilinear and trilinear interpolation reproduce it) and a ball B(x, R) that the
grid covers:  T_1 = b R^2 / 8 (2-D), b R^2 / 10 (3-D), T_k = 0 on the other axes;  U = R^2 f(x) / 4 (2-D), R^2 f(x) / 6 (3-D).
Each estimate of S = 4096 samples lies within 5 of its own standard error; a channel with b = 0 has ds = 0 in every sample, so
its T and seT are 0 exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gradient_source_emulation as gs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WOST_ERR_INVALID = -1
S = 4096
A, B, INTENSITY = (1.5, -0.75, 2.0), (2.0, -3.0, 0.0), 0.7          # per channel; the last has b = 0
# centres and radii: the ball inside [-1, 2]^d, which the grid covers
BALLS = {2: [((0.5, 0.5), 0.3), ((0.2, 0.7), 0.15), ((0.9, 0.1), 0.05), ((-0.3, 1.4), 0.6)],
         3: [((0.5, 0.5, 0.5), 0.3), ((0.2, 0.7, 0.4), 0.15), ((0.9, 0.1, 0.6), 0.05), ((-0.3, 1.4, 0.1), 0.6)]}


def _linear_source(dim):
    """a_c + b_c x on the nodes x = i / 4 - 1, i = 0 .. 12, constant along the other axes"""
    x = np.arange(13) / 4.0 - 1.0
    line = (np.asarray(A)[None, :] + np.asarray(B)[None, :] * x[:, None]).astype(np.float32)          # (nx, 3)
    rgb = np.broadcast_to(line, (13,) * (dim - 1) + (13, 3)).copy()
    src = {"rgb": rgb, "index_scale": (4.0,) * dim, "index_offset": (4.0,) * dim, "intensity": INTENSITY}
    if dim == 2:
        return {"source": src}
    return {"probe": (0.0, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)), "source": src}


def _emulated(oracle, dim):
    pts = np.array([c for c, _ in BALLS[dim]], np.float32)
    R = np.array([r for _, r in BALLS[dim]], np.float32)
    smp = gs.samples(oracle, "linear", _linear_source(dim), pts, R, np.zeros(len(pts), bool), S, 11, 16, dim)
    return pts, R.astype(np.float64), smp, gs.reduce(smp, R)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_in_ball_gradient_term_matches_its_closed_form(oracle, dim):
    pts, R, smp, red = _emulated(oracle, dim)
    want = np.zeros((len(pts), dim, 3))
    want[:, 0, :] = INTENSITY * np.asarray(B)[None, :] * (R * R)[:, None] / (8.0 if dim == 2 else 10.0)
    err, se = np.abs(red["T"] - want), red["seT"]
    print("dim %d: largest |T - closed form| / seT %.3f" % (dim, float((err[:, :, :2] / se[:, :, :2]).max())))
    assert np.all(se[:, :, :2] > 0) and np.all(err <= 5.0 * se), float((err[:, :, :2] / se[:, :, :2]).max())
    # the estimate is no noise: on the axis of the slope it is many of its own standard errors away from 0
    assert np.all(np.abs(red["T"][:, 0, :2]) > 10.0 * se[:, 0, :2])
    # b = 0: the antithetic pair cancels the constant exactly
    assert np.all(smp["ds"][:, :, 2] == 0) and np.all(red["T"][:, :, 2] == 0) and np.all(red["seT"][:, :, 2] == 0)
    assert np.all(smp["ms"][:, :, 2] == np.float32(A[2]) * np.float32(INTENSITY))


@pytest.mark.parametrize("dim", [2, 3])
def test_the_in_ball_field_term_matches_its_closed_form(oracle, dim):
    pts, R, smp, red = _emulated(oracle, dim)
    f = INTENSITY * (np.asarray(A)[None, :] + np.asarray(B)[None, :] * pts[:, :1].astype(np.float64))
    want = (R * R)[:, None] * f / (4.0 if dim == 2 else 6.0)
    err, se = np.abs(red["U"] - want), red["seU"]
    print("dim %d: largest |U - closed form| / seU %.3f" % (dim, float((err / se).max())))
    assert np.all(se > 0) and np.all(err <= 5.0 * se), float((err / se).max())
    assert np.all(np.abs(red["U"]) > 10.0 * se)
    # the weights are bounded: 0 <= wg <= 1, 0 <= wu <= 1 / e (2-D), 1 / 4 (3-D)
    assert smp["wg"].min() >= 0 and smp["wg"].max() <= 1 and smp["wu"].min() >= 0 and smp["wu"].max() <= (0.3679 if dim == 2 else 0.25)


def test_the_in_ball_draws_follow_the_direction_draws(oracle):
    """sample s of a point reads draws (dim - 1) S + dim s .. of the pixel's stream: the jump the kernel makes with pcg_advance"""
    for dim in (2, 3):
        u = gs.draws(oracle, 5, 8, 70, 16, dim)
        r = oracle.pcg_seed_pixel(75, 16)
        oracle.pcg_advance(r, (dim - 1) * 8 + dim * 3)
        assert [np.float32(oracle.pcg_float(r)) for _ in range(dim)] == list(u[3])


# ---- the option door of the C-ABI, no device ---------------------------------------------------------------------------------------
def _fake_handle():
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


def test_wost3_set_option_is_exported_declared_and_prototyped():
    from elaina_amd import capi
    lib = capi.load()
    assert "wost3_set_option" in capi.EXPORTS
    assert lib.wost3_set_option.argtypes == [C.c_void_p, C.c_char_p, C.c_double]
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    assert re.search(r"^int wost3_set_option\(wost3_handle h, const char \*key, double value\);", header, re.M)
    assert "grad_source" in header


@pytest.mark.parametrize("name", ["wost_set_option", "wost3_set_option"])
def test_null_arguments_and_unknown_keys_are_refused(name):
    from elaina_amd import capi
    lib = capi.load()
    fn = getattr(lib, name)
    _keep, handle = _fake_handle()
    assert fn(None, b"grad_source", 1.0) == WOST_ERR_INVALID and b"null argument" in lib.wost_last_error(), lib.wost_last_error()
    assert fn(handle, None, 1.0) == WOST_ERR_INVALID and b"null argument" in lib.wost_last_error(), lib.wost_last_error()
    assert fn(handle, b"grad_sauce", 1.0) == WOST_ERR_INVALID and b"unknown option: grad_sauce" in lib.wost_last_error(), lib.wost_last_error()
    assert _keep.raw == bytes(1 << 16)


@pytest.mark.parametrize("name", ["wost_set_option", "wost3_set_option"])
@pytest.mark.parametrize("value", [0.5, 2.0, -1.0, float("nan")])
def test_grad_source_takes_exactly_0_or_1(name, value):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    assert getattr(lib, name)(handle, b"grad_source", value) == WOST_ERR_INVALID
    assert b"grad_source" in lib.wost_last_error(), lib.wost_last_error()
    assert _keep.raw == bytes(1 << 16)
