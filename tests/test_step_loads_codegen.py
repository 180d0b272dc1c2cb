"""How the walk kernels fetch the tables of a flat Neumann mesh, checked from the gfx950 assembly (tools/kernel_loop_report.py;
no GPU).

A round kernel that refills its lanes stores to global memory inside its scheduler loop, so the compiler cannot prove the
mesh tables unchanged and read the silhouette vertices, their normals and the segment records of the Neumann box with one
vector load per record: 64 lanes, one address, a wait behind each.  With uniform_load (wost_device.h) they are scalar loads.
The counts below are the vector-memory loads inside the loops (in_loop_memory.vector_loads of the report): what the change
reached plus a tenth, and below the count of the commit before it.  The kernels that do not refill issued scalar loads before
and keep their code: their counts are the parent's.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PERSISTENT = "walk_round_kernel<false, false, true, false, false, true>"
REFILL = "walk_round_kernel<false, false, true, false, false, false>"
ROUND = "walk_round_kernel<false, false, false, false, false, false>"
QUAD = "walk_quad_kernel<false, false, false, false>"
QUAD_LONG = "walk_quad_kernel<false, false, false, true>"

# in-loop vector loads: (the commit before, reached by this change)
REFILLING = {PERSISTENT: (65, 42), REFILL: (106, 83),
             "walk_round_kernel<false, false, true, true, false, true>": (80, 50),
             "walk_round_kernel<true, false, true, false, false, true>": (84, 48),
             "walk_round_kernel<true, false, true, false, false, false>": (125, 89),
             "walk_round_kernel<true, false, true, true, false, true>": (99, 56)}
# the kernels that read the tables through the scalar path before: unchanged
UNCHANGED = {ROUND: 66, QUAD: 24, QUAD_LONG: 36}


@pytest.fixture(scope="module")
def kernels():
    import kernel_loop_report
    rep = kernel_loop_report.report("wost_hip.hip", r"walk_(round|quad)_kernel")
    return {k["kernel"].split("(")[0].replace("void wost::", ""): k for k in rep["kernels"]}


@pytest.mark.parametrize("name", sorted(REFILLING))
def test_refilling_kernels_fetch_the_flat_tables_through_the_scalar_path(kernels, name):
    parent, reached = REFILLING[name]
    m = kernels[name]["in_loop_memory"]
    print(name, m, "parent", parent, "budget", int(1.1 * reached))
    assert m["vector_loads"] <= int(1.1 * reached)
    assert m["vector_loads"] < parent
    assert m["scalar_loads"] > 0          # the parent's count was 0: every uniform fetch was a vector load


@pytest.mark.parametrize("name", sorted(UNCHANGED))
def test_other_kernels_keep_their_loads(kernels, name):
    m = kernels[name]["in_loop_memory"]
    print(name, m)
    assert m["vector_loads"] <= UNCHANGED[name]
    assert m["scalar_loads"] > 0


def test_persistent_launch_is_no_larger_than_before(kernels):
    """in-loop instructions, lane moves and waits for vector memory of the persistent instantiation against the commit before"""
    k = kernels[PERSISTENT]
    print(k["in_loop"], k["in_loop_memory"])
    assert k["in_loop"]["instructions"] <= 3306
    assert k["in_loop"]["lane_moves"] <= 225
    assert k["in_loop_memory"]["vmcnt0_waits"] < 42


def test_memory_counts_on_a_small_listing():
    import kernel_loop_report
    body = """
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB0_1:
\tglobal_load_dwordx4 v[0:3], v4, s[0:1]
\ts_load_dwordx4 s[8:11], s[0:1], 0x10
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tbuffer_load_dword v5, v4, s[8:11], 0 offen
\ts_waitcnt vmcnt(0)
\ts_cbranch_scc1 .LBB0_1
\tflat_load_dword v6, v[0:1]
\ts_waitcnt vmcnt(1)
\ts_endpgm
""".strip("\n").split("\n")
    c = kernel_loop_report.count_function(body)
    assert c["memory"] == {"vector_loads": 3, "scalar_loads": 2, "vmcnt0_waits": 2}
    assert c["in_loop_memory"] == {"vector_loads": 2, "scalar_loads": 1, "vmcnt0_waits": 2}


def test_uniform_load_with_a_divergent_address_is_a_per_lane_load(tmp_path):
    """the helper is legal for any address: a wave-uniform one becomes a scalar load, a per-lane one an ordinary vector load"""
    from elaina_amd import build
    src = tmp_path / "probe.hip"
    src.write_text('#include "wost_device.h"\n'
                   "using namespace wost;\n"
                   'extern "C" __global__ void probe_divergent(const float4 *t, float4 *o) { o[threadIdx.x] = uniform_load(t + threadIdx.x); }\n'
                   'extern "C" __global__ void probe_uniform(const float4 *t, float4 *o, int i) { o[threadIdx.x] = uniform_load(t + i); }\n')
    out = tmp_path / "probe.s"
    subprocess.check_call([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
                           "-I", build.CSRC, str(src), "-o", str(out)], stderr=subprocess.DEVNULL)
    text = out.read_text()
    div = text[text.index("probe_divergent:"):text.index("probe_uniform:")]
    uni = text[text.index("probe_uniform:"):]
    uni = uni[:uni.index("s_endpgm")]
    assert "global_load_dwordx4" in div
    assert "global_load" not in uni and uni.count("s_load_dwordx4") >= 2      # the arguments, then the table
