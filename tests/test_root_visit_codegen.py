"""How the walk kernels fetch the root of the Dirichlet tree at query start (wost_device.h: trav_visit_root), checked from the
gfx950 assembly (tools/kernel_loop_report.py; no GPU).

The root visit of the step phase reads the root's six rows on the scalar path and leaves out the leaf-level part of a visit,
so the kernels gain scalar loads and no vector load: the 16-byte node gathers are those of the traversal bursts alone, and the
segOrig fetches of the tie path are not duplicated.  The parent's figures are those of profiles/kernel_loop_report_parent.json,
regenerated on the commit before this change (its gathers counted from the same assembly).
"""
import os
import re
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PERSISTENT = "walk_round_kernel<false, false, true, false, false, true>"
ROUND = "walk_round_kernel<false, false, false, false, false, false>"

# the commit before: in-loop vector loads, in-loop scalar loads, in-loop global_load_dwordx4
PARENT = {PERSISTENT: dict(vector_loads=42, scalar_loads=16, dwordx4=8),
          ROUND: dict(vector_loads=66, scalar_loads=23, dwordx4=26)}

_OTHER_VECTOR_LOAD = re.compile(r"^\s+(global|flat|buffer)_load_(?!dwordx4\b)")


def _name(pretty):
    return pretty.split("(")[0].replace("void wost::", "")


@pytest.fixture(scope="module")
def kernels():
    import kernel_loop_report as rep
    asm, _ = rep.assembly("wost_hip.hip")
    bodies = rep.function_bodies(open(asm).read())
    pretty = rep.demangle(list(bodies))
    out = {}
    for sym, body in bodies.items():
        name = _name(pretty[sym])
        if name not in PARENT:
            continue
        counts = rep.count_function(body)
        # the 16-byte gathers alone: the same listing with every other vector load blanked, so the loops are the same loops
        only_x4 = rep.count_function([("\ts_nop 0" if _OTHER_VECTOR_LOAD.match(line) else line) for line in body])
        out[name] = dict(counts["in_loop_memory"], dwordx4=only_x4["in_loop_memory"]["vector_loads"])
    assert sorted(out) == sorted(PARENT)
    return out


def test_persistent_launch_reads_the_root_on_the_scalar_path(kernels):
    m, p = kernels[PERSISTENT], PARENT[PERSISTENT]
    print(PERSISTENT, m, "parent", p)
    assert m["dwordx4"] <= p["dwordx4"]
    assert m["scalar_loads"] > p["scalar_loads"]


def test_round_kernel_keeps_its_own_scalar_loads(kernels):
    m, p = kernels[ROUND], PARENT[ROUND]
    print(ROUND, m, "parent", p)
    assert m["scalar_loads"] >= p["scalar_loads"]
    assert m["vector_loads"] <= int(1.1 * p["vector_loads"])


def test_gathers_are_told_from_other_loads_on_a_small_listing():
    import kernel_loop_report as rep
    body = """
.LBB0_1:
\tglobal_load_dwordx4 v[0:3], v4, s[0:1]
\tglobal_load_dword v5, v4, s[0:1]
\tglobal_load_dwordx2 v[6:7], v4, s[0:1]
\ts_load_dwordx16 s[8:23], s[0:1], 0x0
\ts_cbranch_scc1 .LBB0_1
\tglobal_load_dwordx4 v[0:3], v4, s[0:1]
\ts_endpgm
""".strip("\n").split("\n")
    blanked = [("\ts_nop 0" if _OTHER_VECTOR_LOAD.match(line) else line) for line in body]
    assert rep.count_function(body)["in_loop_memory"]["vector_loads"] == 3
    c = rep.count_function(blanked)
    assert c["in_loop_memory"]["vector_loads"] == 1 and c["memory"]["vector_loads"] == 2
    assert c["in_loop_memory"]["scalar_loads"] == 1
