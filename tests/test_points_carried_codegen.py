"""What the carried point list did to the walk kernels, from the gfx950 assembly (tools/kernel_loop_report.py; no GPU): the 3-D
walk kernel has sixteen more instantiations, those with POINTS and CARRY both set, and the 2-D walk kernels none -- a carried
point is resolved by the entries a carried pixel is resolved by."""
import os
import re
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# The walk_round* / walk_quad* entries of wost_hip.hip on the commit before the carried point list: per entry the template
# arguments of its instantiations, one digit per bool (1 = true), as tools/kernel_loop_report.py listed them there.
PARENT_ENTRIES_2D = {
    "walk_quad_carry_kernel": "0000 0001 0010 0011 0100 0101 0110 0111 1000 1001 1010 1011 1100 1101 1110 1111",
    "walk_quad_kernel": "0000 0001 0010 0011 0100 0101 0110 0111 1000 1001 1010 1011 1100 1101 1110 1111",
    "walk_round_carry_kernel": "000000 000010 000100 000110 001000 001001 001101 010000 010010 010100 010110 011000 011001 011101 100000 100010 100100 100110 101000 101001 101101 110000 110010 110100 110110 111000 111001 111101",
    "walk_round_kernel": "000000 000010 000100 000110 001000 001001 001101 010000 010010 010100 010110 011000 011001 011101 100000 100010 100100 100110 101000 101001 101101 110000 110010 110100 110110 111000 111001 111101",
}


def _names(source, match):
    """the kernels of csrc/<source> that the report lists under `match` (its steps without the instruction counts, which take a
    minute on the 3-D kernels and are not needed here)"""
    import kernel_loop_report as klr
    asm, remarks = klr.assembly(source)
    res = klr.parse_remarks(open(remarks).read())
    symbols = [n for n in klr.function_bodies(open(asm).read()) if n in res]
    pretty = klr.demangle(symbols)
    pat = re.compile(match)
    return [pretty[n].split("(")[0].replace("void wost::", "") for n in symbols if pat.search(n) or pat.search(pretty[n])]


def _flags(name):
    return [a.strip() == "true" for a in re.search(r"<(.*)>", name).group(1).split(",")]


def test_walk3_kernel_has_sixteen_more_instantiations_for_points_that_carry():
    names = [n for n in _names("wost_hip3d.hip", r"walk3_kernel") if n.startswith("walk3_kernel<")]
    assert len(names) == len(set(names)) == 64
    flags = [_flags(n) for n in names]
    assert all(len(f) == 6 for f in flags)
    both = [f for f in flags if f[4] and f[5]]
    assert len(both) == 16 and len({tuple(f[:4]) for f in both}) == 16
    # ... beside the sixteen of each form there was: frame, POINTS, frame CARRY
    for points, carry in ((False, False), (True, False), (False, True)):
        assert sum(1 for f in flags if f[4] == points and f[5] == carry) == 16


def test_the_2d_walk_entries_are_those_of_the_parent_commit():
    names = _names("wost_hip.hip", r"walk_(round|quad)")
    assert len(names) == len(set(names))
    want = {"%s<%s>" % (entry, ", ".join("true" if d == "1" else "false" for d in args))
            for entry, lists in PARENT_ENTRIES_2D.items() for args in lists.split()}
    assert len(want) == 88
    assert set(names) == want, (sorted(set(names) - want), sorted(want - set(names)))
