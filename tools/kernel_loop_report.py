#!/usr/bin/env python3
"""Static report of what a kernel's loops cost in instructions that the result does not need.

Compiles one csrc/*.hip to gfx950 assembly with the flags of elaina_amd/build.py (device code only: no GPU is needed) and
prints, for every kernel whose (mangled or demangled) name matches a pattern, one JSON object:

  vgprs, sgprs, agprs, sgpr_spills, vgpr_spills, scratch_bytes, occupancy, lds_bytes   (-Rpass-analysis=kernel-resource-usage)
  instructions                                   static instruction count
  v_mov, lane_moves, scratch                     v_mov_*, v_readlane/v_writelane and scratch_* among them
  in_loop: {instructions, v_mov, lane_moves, scratch}   the same counts over the basic blocks that lie inside a loop
  memory, in_loop_memory: {vector_loads, scalar_loads, vmcnt0_waits}
                                                 global_/flat_/buffer_load_*, s_load_*/s_buffer_load_* and the s_waitcnt that
                                                 wait for vmcnt(0), over the kernel and over the blocks inside a loop
  loop_list                                      every loop on its own: position, nesting depth, instructions and v_mov with
                                                 and without the loops nested inside it

A block lies inside a loop when it stands between a label and a later branch that jumps back to that label.  The counts are
static: they say what the loops contain, not how often a path runs.  The register copies between the two homes the compiler
gives a loop-carried value (EXPERIMENTS "Register copies around the scheduler loop") show up as in_loop.v_mov.

    python tools/kernel_loop_report.py                       # the walk kernels of wost_hip.hip
    python tools/kernel_loop_report.py wost_hip3d.hip --match walk3

The assembly is kept under elaina_amd/lib/asm/, keyed by the source id and the flags, so a second report of the same tree
costs nothing (a compile of wost_hip.hip takes over a minute).
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from elaina_amd import build as _build  # noqa: E402

ASM_DIR = os.path.join(_build.LIB_DIR, "asm")

_REMARK = re.compile(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]")
_FIELDS = {
    "TotalSGPRs": "sgprs", "SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes",
    "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sgpr_spills", "VGPRs Spill": "vgpr_spills",
    "LDS Size [bytes/block]": "lds_bytes",
}
_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_BRANCH = re.compile(r"^\s+s_c?branch\S*\s+(\.LBB\d+_\d+)\b")
_INSTR = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")


def compile_flags():
    """the device-side flags of the library build (no -shared: nothing is linked)"""
    return [f for f in _build.HIPCC_FLAGS if f != "-shared"] + os.environ.get("WOST_HIPCC_DEFS", "").split()


def assembly(source, force=False, verbose=False):
    """paths of the assembly and the resource remarks of csrc/<source>, compiled when the cache has neither"""
    flags = compile_flags()
    key = hashlib.sha256((_build.source_id() + " " + source + " " + " ".join(flags)).encode()).hexdigest()[:16]
    stem = os.path.join(ASM_DIR, "%s.%s" % (os.path.splitext(source)[0], key))
    asm, remarks = stem + ".s", stem + ".remarks"
    if force or not (os.path.exists(asm) and os.path.exists(remarks)):
        os.makedirs(ASM_DIR, exist_ok=True)
        cmd = [_build._hipcc()] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                           os.path.join(_build.CSRC, source), "-o", asm + ".tmp"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise subprocess.CalledProcessError(p.returncode, cmd)
        with open(remarks, "w") as f:
            f.write(p.stderr)
        os.replace(asm + ".tmp", asm)
    return asm, remarks


def parse_remarks(text):
    """{mangled kernel name: {field: int}} from the compiler's kernel-resource-usage remarks"""
    out, cur = {}, None
    for line in text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        body = m.group(1)
        if body.startswith("Function Name:"):
            cur = out.setdefault(body.split(":", 1)[1].strip(), {})
            continue
        if cur is None or ":" not in body:
            continue
        name, value = body.rsplit(":", 1)
        field = _FIELDS.get(name.strip())
        if field is not None:
            try:
                cur[field] = int(value)
            except ValueError:
                pass
    return out


def function_bodies(asm_text):
    """{symbol: [lines]} of every function of the assembly: from its label to its .Lfunc_end"""
    out, name, body = {}, None, None
    for line in asm_text.splitlines():
        if name is None:
            m = re.match(r"^\s+\.type\s+(\S+),@function", line)
            if m:
                name, body = m.group(1), None
            continue
        if body is None:
            if line.startswith(name + ":"):
                body = []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name, body = None, None
            continue
        body.append(line)
    return out


def _kind(op):
    if op.startswith("v_mov_"):
        return "v_mov"
    if op.startswith(("v_readlane", "v_writelane")):
        return "lane_moves"
    if op.startswith("scratch_"):
        return "scratch"
    return None


_VMCNT0 = re.compile(r"\bvmcnt\(0\)")


def _memory_kind(op, line):
    """vector_loads / scalar_loads / vmcnt0_waits, or None: what brings operands in and what waits for them"""
    if op.startswith(("global_load_", "flat_load_", "buffer_load_")):
        return "vector_loads"
    if op.startswith(("s_load_", "s_buffer_load_")):
        return "scalar_loads"
    if op == "s_waitcnt" and _VMCNT0.search(line):
        return "vmcnt0_waits"
    return None


def count_function(lines):
    """static instruction counts of one function body, whole and restricted to the blocks inside a loop"""
    label_at = {}
    instrs = []          # (line index, opcode)
    branches = []        # (line index, target label)
    for i, line in enumerate(lines):
        m = _LABEL.match(line)
        if m:
            label_at[m.group(1)] = i
            continue
        m = _INSTR.match(line)
        if not m or line.lstrip().startswith((".", ";")):
            continue
        instrs.append((i, m.group(1)))
        b = _BRANCH.match(line)
        if b:
            branches.append((i, b.group(1)))
    # a back edge: a branch to a label that stands before it.  Everything between the two is inside that loop.
    spans = sorted((label_at[t], i) for i, t in branches if t in label_at and label_at[t] < i)
    merged = []
    for lo, hi in spans:
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])

    def inside(i):
        return any(lo <= i <= hi for lo, hi in merged)

    total = {"instructions": 0, "v_mov": 0, "lane_moves": 0, "scratch": 0}
    loop = dict(total)
    mem = {"vector_loads": 0, "scalar_loads": 0, "vmcnt0_waits": 0}
    loop_mem = dict(mem)
    for i, op in instrs:
        k = _kind(op)
        mk = _memory_kind(op, lines[i])
        for d, md in ([(total, mem), (loop, loop_mem)] if inside(i) else [(total, mem)]):
            d["instructions"] += 1
            if k:
                d[k] += 1
            if mk:
                md[mk] += 1
    total["in_loop"] = loop
    # beside in_loop, not inside it: the four counts of in_loop are compared as a whole by tests/test_kernel_codegen.py
    total["memory"] = mem
    total["in_loop_memory"] = loop_mem
    total["loops"] = len(merged)
    # every loop on its own (spans that share a head are one loop with several back edges): where it starts, as the number of
    # instructions before its head, how deep it is nested, and what it holds -- `own` without the loops nested inside it.
    # This is what a path is judged by: the copies a trip of the traversal loop pays are the v_mov of that loop alone.
    heads = {}
    for lo, hi in spans:
        heads[lo] = max(heads.get(lo, hi), hi)
    each = sorted(heads.items())
    detail = []
    for lo, hi in each:
        inner = [(a, b) for a, b in each if (a, b) != (lo, hi) and lo <= a and b <= hi]
        row = {"first_instruction": sum(1 for i, _ in instrs if i < lo), "depth": sum(1 for a, b in each if a <= lo and hi <= b),
               "instructions": 0, "v_mov": 0, "own_instructions": 0, "own_v_mov": 0}
        for i, op in instrs:
            if lo <= i <= hi:
                own = not any(a <= i <= b for a, b in inner)
                mov = _kind(op) == "v_mov"
                row["instructions"] += 1
                row["v_mov"] += mov
                row["own_instructions"] += own
                row["own_v_mov"] += mov and own
        detail.append(row)
    total["loop_list"] = detail
    return total


def demangle(names):
    try:
        p = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, universal_newlines=True, check=True)
        d = p.stdout.splitlines()
        if len(d) == len(names):
            return dict(zip(names, d))
    except (OSError, subprocess.CalledProcessError):
        pass
    return {n: n for n in names}


def report(source="wost_hip.hip", match=r"walk_(round|quad)_kernel", force=False, verbose=False):
    """list of per-kernel dicts for the kernels of csrc/<source> whose name matches"""
    asm, remarks = assembly(source, force=force, verbose=verbose)
    res = parse_remarks(open(remarks).read())
    bodies = function_bodies(open(asm).read())
    pat = re.compile(match)
    names = [n for n in bodies if n in res]
    pretty = demangle(names)
    out = []
    for n in names:
        if not (pat.search(n) or pat.search(pretty[n])):
            continue
        row = {"kernel": pretty[n], "symbol": n}
        row.update(res[n])
        row.update(count_function(bodies[n]))
        out.append(row)
    return {"source": source, "source_id": _build.source_id(), "flags": compile_flags(), "kernels": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("source", nargs="?", default="wost_hip.hip", help="a file of elaina_amd/csrc")
    ap.add_argument("--match", default=r"walk_(round|quad)_kernel", help="regular expression on the kernel's name")
    ap.add_argument("--force", action="store_true", help="compile even when the assembly is cached")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--summary", action="store_true", help="leave out the list of single loops (the form committed under profiles/)")
    ap.add_argument("-o", "--output", help="write the JSON here instead of standard output")
    a = ap.parse_args()
    rep = report(a.source, a.match, a.force, a.verbose)
    if a.summary:
        for k in rep["kernels"]:
            del k["loop_list"]
    text = json.dumps(rep, indent=1)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
