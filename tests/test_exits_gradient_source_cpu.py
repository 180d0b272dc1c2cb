"""The in-ball term of an exit list of the gradient without a GPU: the join of exits_gradient_source_emulation.py on synthetic
records (exits_gradient_emulation.synthetic), and the doors of the C-ABI that need no device -- the option "exits_grad_source" of
wost_set_option and wost3_set_option on the zeroed block of memory tests/test_gradient_source_cpu.py uses in place of a handle,
the new exports and their prototypes, the reader's null handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exits_gradient_emulation as xg
import exits_gradient_source_emulation as xs
from test_gradient_source_cpu import WOST_ERR_INVALID, _fake_handle

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS, INTENSITY = 1e-3, 1.25


def _list(dim, n=9, S=11, n_prims=14, seed=3):
    """a synthetic list with two degenerate points (a radius inside the shell, a NaN one), a set of colours and its walk part"""
    rng = np.random.default_rng(seed)
    rec, grec = xg.synthetic(rng, n, S, n_prims, dim)
    grec["radius"][1], grec["radius"][4] = np.float32(0.5 * EPS), np.float32(np.nan)
    prims = rng.integers(0, 10, size=(n_prims, dim)).astype(np.int32)
    colors = rng.uniform(-1.0, 2.0, size=(2, 10, 6)).astype(np.float32)
    walk = xg.apply(rec, grec, colors, prims, INTENSITY, EPS, dim)
    terms = (rng.normal(size=(n, dim, 3)), np.abs(rng.normal(size=(n, dim, 3))), rng.normal(size=(n, 3)))
    return rec, grec, prims, colors, walk, terms, xg.degenerate(grec["radius"], EPS)


@pytest.mark.parametrize("dim", [2, 3])
def test_zero_terms_return_the_bits_of_the_walk_part(dim):
    rec, grec, prims, colors, walk, _, deg = _list(dim)
    assert deg.sum() == 2
    n = len(deg)
    zero = (np.zeros((n, dim, 3)), np.zeros((n, dim, 3)), np.zeros((n, 3)))
    got = xs.apply(rec, grec, colors, prims, INTENSITY, EPS, dim, *zero)
    for k in ("grad", "stderr", "field"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k], walk[k].astype(np.float32), equal_nan=True), k
    assert np.all(np.isfinite(got["grad"][:, ~deg])) and np.any(got["grad"][:, ~deg] != 0)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_join_adds_T_and_U_and_takes_the_root_of_the_sum_of_squares(dim):
    rec, grec, prims, colors, walk, (T, seT, U), deg = _list(dim)
    got = xs.apply(rec, grec, colors, prims, INTENSITY, EPS, dim, T, seT, U)
    ok = ~deg
    for k in range(len(colors)):
        assert np.array_equal(got["grad"][k][ok], (walk["grad"][k][ok] + T[ok]).astype(np.float32))
        assert np.array_equal(got["stderr"][k][ok], np.sqrt(walk["stderr"][k][ok] ** 2 + seT[ok] ** 2).astype(np.float32))
        assert np.array_equal(got["field"][k][ok], (walk["field"][k][ok] + U[ok]).astype(np.float32))
        # no smaller than either part, no larger than their sum
        se = got["stderr"][k][ok].astype(np.float64)
        lo, hi = np.maximum(walk["stderr"][k][ok], seT[ok]), walk["stderr"][k][ok] + seT[ok]
        assert np.all(se >= lo * (1 - 2.0 ** -23)) and np.all(se <= hi * (1 + 2.0 ** -23))
    # the same terms in every set: the difference of two sets is that of their walk parts, up to the two roundings to float32
    d_got = got["grad"][0][ok].astype(np.float64) - got["grad"][1][ok]
    d_walk = walk["grad"][0][ok] - walk["grad"][1][ok]
    assert np.all(np.abs(d_got - d_walk) <= 2.0 ** -23 * (np.abs(got["grad"][0][ok]) + np.abs(got["grad"][1][ok])))


@pytest.mark.parametrize("dim", [2, 3])
def test_a_degenerate_point_gets_nan_nan_and_its_mean_without_U(dim):
    rec, grec, prims, colors, walk, (T, seT, U), deg = _list(dim)
    got = xs.apply(rec, grec, colors, prims, INTENSITY, EPS, dim, T, seT, U)
    assert deg[1] and deg[4] and np.all(U[deg] != 0)
    for k in range(len(colors)):
        assert np.all(np.isnan(got["grad"][k][deg])) and np.all(np.isnan(got["stderr"][k][deg]))
        assert np.array_equal(got["field"][k][deg], walk["field"][k][deg].astype(np.float32)) and np.all(np.isfinite(got["field"][k][deg]))


# ---- the doors of the C-ABI, no device ---------------------------------------------------------------------------------------------
def test_the_new_names_are_exported_declared_and_prototyped():
    from elaina_amd import capi
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    pd = C.POINTER(C.c_double)
    for prefix, handle in (("wost_", "wost_handle"), ("wost3_", "wost3_handle")):
        name = prefix + "exits_gradient_terms"
        assert name in capi.EXPORTS
        assert getattr(lib, name).argtypes == [C.c_void_p, pd, pd, pd]
        assert re.search(r"^int %s\(%s h, double \*T, double \*seT, double \*U\);" % (name, handle), header, re.M), name
    assert header.count("exits_grad_source") >= 4


@pytest.mark.parametrize("name", ["wost_set_option", "wost3_set_option"])
@pytest.mark.parametrize("value", [0.5, 2.0, -1.0, float("nan")])
def test_exits_grad_source_takes_exactly_0_or_1(name, value):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    assert getattr(lib, name)(handle, b"exits_grad_source", value) == WOST_ERR_INVALID
    assert b"exits_grad_source" in lib.wost_last_error(), lib.wost_last_error()
    assert _keep.raw == bytes(1 << 16)


@pytest.mark.parametrize("name", ["wost_set_option", "wost3_set_option"])
def test_the_option_is_a_key_of_its_own_and_unknown_keys_are_still_refused(name):
    from elaina_amd import capi
    lib = capi.load()
    fn = getattr(lib, name)
    _keep, handle = _fake_handle()
    for key in (b"exits_grad_sauce", b"exits_grad_source ", b"exits_grad"):
        assert fn(handle, key, 1.0) == WOST_ERR_INVALID and b"unknown option: " + key in lib.wost_last_error(), lib.wost_last_error()
    assert _keep.raw == bytes(1 << 16)
    # 0 on a zeroed block writes what is there; 1 sets one byte, and it is not the byte of "grad_source"
    assert fn(handle, b"exits_grad_source", 0.0) == 0 and _keep.raw == bytes(1 << 16)
    assert fn(handle, b"exits_grad_source", 1.0) == 0
    mine = [i for i, b in enumerate(_keep.raw) if b]
    assert len(mine) == 1 and _keep.raw[mine[0]] == 1
    assert fn(handle, b"exits_grad_source", 0.0) == 0 and _keep.raw == bytes(1 << 16)
    assert fn(handle, b"grad_source", 1.0) == 0
    other = [i for i, b in enumerate(_keep.raw) if b]
    assert len(other) == 1 and other != mine


@pytest.mark.parametrize("name", ["wost_exits_gradient_terms", "wost3_exits_gradient_terms"])
def test_the_reader_refuses_a_null_handle(name):
    from elaina_amd import capi
    lib = capi.load()
    out = np.full(9, -1.0)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    for args in ((None, None, None), (p, None, None), (p, p, p)):
        assert getattr(lib, name)(None, *args) == WOST_ERR_INVALID and b"null argument" in lib.wost_last_error(), lib.wost_last_error()
    assert np.all(out == -1.0)
