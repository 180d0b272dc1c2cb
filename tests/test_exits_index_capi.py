"""The index of the exit list and the ordered adjoints in the C-ABI (wost_exits_index, _index_info, _index_records,
_adjoint_ordered, _adjoint_ordered_dev, _adjoint_gradient_ordered, _adjoint_gradient_ordered_dev and their wost3_ forms) without
a GPU: the fourteen names exist, include/wost.h declares them under its own heading, Python knows their prototypes and the
integrator front end has the methods, and every argument that can be refused before a device is asked for is refused with
WOST_ERR_INVALID, in the order of the header, with a message that names the quantity and the outputs untouched.  (The handle is
a block of zeroed memory: none of these refusals may read more of it than the fact that it holds no list and no index.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N_ARGS = {"exits_index": 1, "exits_index_info": 3, "exits_index_records": 3, "exits_adjoint_ordered": 4, "exits_adjoint_ordered_dev": 5,
          "exits_adjoint_gradient_ordered": 4, "exits_adjoint_gradient_ordered_dev": 5}
PREFIXES = ["wost_", "wost3_"]
NAMES = [pre + f for pre in PREFIXES for f in N_ARGS]
WOST_ERR_INVALID = -1


def _fake_handle():
    fake = C.create_string_buffer(1 << 16)
    return fake, C.c_void_p(C.addressof(fake))


def test_there_are_fourteen_names_a_heading_and_the_methods():
    from elaina_amd import uniform
    assert len(NAMES) == len(set(NAMES)) == 14
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    heading = "Exit lists: the index and the ordered adjoint"
    assert heading in header and header.index(heading) > header.index("/* Exit lists of the gradient (DESIGN 4.3i)")
    # the contract states the promise and the order a caller needs to reproduce the bits
    section = header[header.index(heading):header.index("int wost_exits_index(")]
    for word in ("SAME BITS ON EVERY RUN", "ascending", "32, 16, 8, 4, 2, 1", "+0.0", "SKIPPED", "wost_exits_walk_gradient", "WOST_ERR_UNSUPPORTED"):
        assert word in section, word
    methods = ["exits_index", "exits_index_info", "exits_index_records", "exits_adjoint_ordered", "exits_adjoint_ordered_dev",
               "exits_adjoint_gradient_ordered", "exits_adjoint_gradient_ordered_dev"]
    owners = [c for c in vars(uniform).values() if isinstance(c, type) and hasattr(c, "exits_adjoint")]
    assert owners and all(hasattr(c, m) for c in owners for m in methods)


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_are_exported_declared_and_prototyped(name):
    from elaina_amd import capi
    lib = capi.load()
    assert name in capi.EXPORTS
    fn = getattr(lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == N_ARGS[name.split("_", 1)[1]]
    header = open(os.path.join(ROOT, "include", "wost.h")).read()
    m = re.search(r"^int %s\((wost3?_handle h[^;]*)\);" % name, header, re.M | re.S)
    assert m, name
    assert m.group(1).count(",") + 1 == N_ARGS[name.split("_", 1)[1]], m.group(1)
    assert m.group(1).startswith("wost3_handle" if name.startswith("wost3_") else "wost_handle")


@pytest.mark.parametrize("pre", PREFIXES)
def test_a_handle_without_a_list_has_no_index_and_builds_none(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    g = lambda name: getattr(lib, pre + "exits_" + name)
    n_inc, longest = C.c_int64(-5), C.c_int64(-5)
    assert g("index_info")(handle, C.byref(n_inc), C.byref(longest)) == 0 and (n_inc.value, longest.value) == (0, 0)
    begin, inc = np.full(8, -1, np.int64), np.full(8, -1, np.int32)
    pb, pi = begin.ctypes.data_as(C.POINTER(C.c_int64)), capi._ip(inc)
    n_inc.value = -5
    calls = [
        (lambda: g("index")(None), b"null"),
        (lambda: g("index")(handle), b"no exit list is bound"),
        (lambda: g("index_info")(None, C.byref(n_inc), C.byref(n_inc)), b"null"),
        (lambda: g("index_info")(handle, None, C.byref(n_inc)), b"null"),
        (lambda: g("index_info")(handle, C.byref(n_inc), None), b"null"),
        (lambda: g("index_records")(None, pb, pi), b"null"),
        (lambda: g("index_records")(handle, pb, pi), b"no exit list is bound"),
        (lambda: g("index_records")(handle, None, None), b"no exit list is bound"),
    ]
    for k, (call, word) in enumerate(calls):
        assert call() == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    assert n_inc.value == -5 and np.all(begin == -1) and np.all(inc == -1)


@pytest.mark.parametrize("pre", PREFIXES)
def test_the_ordered_adjoints_refuse_null_arrays_a_bad_k_and_a_handle_without_a_list(pre):
    from elaina_amd import capi
    lib = capi.load()
    _keep, handle = _fake_handle()
    colors, d = (np.full(54, -1.0, np.float32) for _ in range(2))
    c, f = capi._fp(colors), capi._fp(d)
    dc, df = (C.c_void_p(a.ctypes.data) for a in (colors, d))
    g = lambda name: getattr(lib, pre + "exits_" + name)
    # every row breaks the rule it names and the rules after it (K = 0, and the zeroed handle holds no list and no index)
    calls = []
    for form, arg in (("adjoint_ordered", b"dfield"), ("adjoint_gradient_ordered", b"dgrad")):
        calls += [
            (lambda form=form: g(form)(None, f, 0, c), b"null"),
            (lambda form=form: g(form)(handle, None, 0, c), b"null argument: " + arg),
            (lambda form=form: g(form)(handle, f, 0, None), b"null argument: dcolors"),
            (lambda form=form: g(form)(handle, f, 0, c), b"K must be at least 1"),
            (lambda form=form: g(form)(handle, f, -1, c), b"K must be at least 1"),
            (lambda form=form: g(form)(handle, f, 2, c), b"no exit list is bound"),
            (lambda form=form: g(form + "_dev")(None, df, 0, dc, None), b"null"),
            (lambda form=form: g(form + "_dev")(handle, None, 0, dc, None), b"null argument: " + arg),
            (lambda form=form: g(form + "_dev")(handle, df, 0, None, None), b"null argument: dcolors"),
            (lambda form=form: g(form + "_dev")(handle, df, 0, dc, None), b"K must be at least 1"),
            (lambda form=form: g(form + "_dev")(handle, df, 1, dc, None), b"no exit list is bound"),
        ]
    for k, (call, word) in enumerate(calls):
        assert call() == WOST_ERR_INVALID and word in lib.wost_last_error(), (k, lib.wost_last_error())
    assert all(np.all(a == -1.0) for a in (colors, d))
