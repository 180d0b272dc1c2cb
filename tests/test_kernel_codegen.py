"""What the compiler makes of the walk kernels, checked from the gfx950 assembly (tools/kernel_loop_report.py; no GPU).

The two instantiations that carry config 2 -- the persistent first launch and the plain round -- are VALU-bound at six waves per
SIMD, so three things about their code are worth a failing test: the resources that decide the occupancy,
the scratch a lane spills to, and the register copies inside the loops (the lane state moved between the two homes the
compiler gives it; EXPERIMENTS "Register copies around the scheduler loop").  The limits on the resources are the figures of
the kernels before that work; the copy budgets are what it reached plus a tenth.
"""
import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PERSISTENT = "walk_round_kernel<false, false, true, false, false, true>"
ROUND = "walk_round_kernel<false, false, false, false, false, false>"

# in-loop v_mov reached by the change that introduced this test, plus a tenth (int(1.1 * reached))
COPY_BUDGET = {PERSISTENT: int(1.1 * 308), ROUND: int(1.1 * 314)}


@pytest.fixture(scope="module")
def kernels():
    import kernel_loop_report
    rep = kernel_loop_report.report("wost_hip.hip", r"walk_round_kernel")
    return {k["kernel"].split("(")[0].replace("void wost::", ""): k for k in rep["kernels"]}


def test_report_finds_the_kernels_and_their_loops(kernels):
    for name in (PERSISTENT, ROUND):
        k = kernels[name]
        assert k["instructions"] > 1000 and k["loops"] >= 1
        assert 0 < k["in_loop"]["instructions"] <= k["instructions"]
        assert k["in_loop"]["v_mov"] <= k["v_mov"]
        assert all(l["own_v_mov"] <= l["v_mov"] <= l["instructions"] for l in k["loop_list"])


def test_persistent_launch_keeps_its_occupancy(kernels):
    k = kernels[PERSISTENT]
    print({f: k[f] for f in ("vgprs", "sgprs", "occupancy", "scratch_bytes", "lds_bytes", "sgpr_spills", "vgpr_spills")})
    # EXPERIMENTS section 25: 259 / 234 / 222 ms at 4 / 5 / 6 blocks per CU
    assert k["occupancy"] >= 6
    assert k["vgprs"] <= 80
    assert k["scratch_bytes"] <= 48
    assert k["lds_bytes"] == 68        # the static words of block_push; the stack columns are dynamic


def test_round_kernel_keeps_its_occupancy(kernels):
    k = kernels[ROUND]
    print({f: k[f] for f in ("vgprs", "sgprs", "occupancy", "scratch_bytes", "lds_bytes", "sgpr_spills", "vgpr_spills")})
    assert k["occupancy"] >= 6
    assert k["vgprs"] <= 80
    assert k["lds_bytes"] == 68


@pytest.mark.parametrize("name", [PERSISTENT, ROUND])
def test_register_copies_inside_the_loops_stay_within_budget(kernels, name):
    k = kernels[name]
    print(name, "in-loop v_mov", k["in_loop"]["v_mov"], "of", k["in_loop"]["instructions"], "budget", COPY_BUDGET[name])
    assert k["in_loop"]["v_mov"] <= COPY_BUDGET[name]


def test_loop_detection_on_a_small_listing():
    import kernel_loop_report
    body = """
\ts_mov_b32 s0, 0
.LBB0_1:
\tv_mov_b32_e32 v1, v0
\tv_add_u32_e32 v0, 1, v1
.LBB0_2:
\tv_mov_b32_e32 v2, v0
\ts_cbranch_scc1 .LBB0_2
\tv_readlane_b32 s1, v3, 0
\ts_cbranch_vccnz .LBB0_1
\tv_mov_b32_e32 v4, v2
\tscratch_store_dword off, v4, off
\ts_endpgm
""".strip("\n").split("\n")
    c = kernel_loop_report.count_function(body)
    assert c["instructions"] == 10 and c["v_mov"] == 3 and c["lane_moves"] == 1 and c["scratch"] == 1
    assert c["in_loop"] == {"instructions": 6, "v_mov": 2, "lane_moves": 1, "scratch": 0}
    assert [(l["depth"], l["instructions"], l["own_instructions"], l["v_mov"], l["own_v_mov"]) for l in c["loop_list"]] == \
        [(1, 6, 4, 2, 1), (2, 2, 2, 1, 1)]
