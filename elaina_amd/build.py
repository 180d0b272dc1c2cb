"""Build the HIP shared library (libwost_hip.so) for gfx950, in-tree.

hipcc cross-compiles without a GPU, so this runs in the build container as the
"does it build" check and the resulting .so travels to the GPU box with the tree.
"""
import hashlib
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libwost_hip.so")
HOST_EXE = os.path.join(LIB_DIR, "elaina-exec")
OBJ_DIR = os.path.join(LIB_DIR, "obj")

SOURCES = ["wost_hip.hip", "wost_order.hip", "wost_carry.hip", "wost_grad.hip", "wost_grad_carry.hip", "wost_exits.hip", "wost_exits_index.hip", "wost_hip3d.hip", "wost_build2.hip", "wost_build3.hip", "wost_vmm3.hip", "wost_guided3.hip", "wost_vmm.hip", "wost_net.hip", "wost_train.hip", "wost_guided.hip", "lbvh_build.cpp"]

# -ffp-contract=off is part of the arithmetic contract (DESIGN.md "deterministic math")
HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
    "-Wall", "-Wno-unused-function",
]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP library cannot be built")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build_library(force=False, verbose=False):
    """One object per translation unit (compiled in parallel, rebuilt when the unit or ANY header
    of csrc/ or include/wost.h is newer, or when the compiler flags differ from those the objects
    were built with), then one link."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")]
    headers.append(os.path.join(_HERE, "..", "include", "wost.h"))
    # developer knob: extra -D definitions for kernel-tuning experiments (WOST_HIPCC_DEFS="-DX=1 -DY=2")
    flags = _library_flags()
    # objects are only reused under the flags they were compiled with: a library carrying experimental -D variants must
    # never be mistaken for the default build by the next plain build (and the other way round)
    stamp = os.path.join(OBJ_DIR, "flags.stamp")
    flag_id = hashlib.sha256(" ".join(flags).encode()).hexdigest()
    try:
        same_flags = open(stamp).read().strip() == flag_id
    except OSError:
        same_flags = False
    if not same_flags:
        force = True
    jobs, objs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ_DIR, os.path.splitext(s)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + headers):
            cmd = [_hipcc()] + flags + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd)))
    # wait for every compiler before reporting a failure: none is left running behind an exception
    failed = [(cmd, p.returncode) for cmd, p in jobs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(failed[0][1], failed[0][0])
    with open(stamp, "w") as f:
        f.write(flag_id + "\n")
    if force or jobs or _stale(LIB_PATH, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", LIB_PATH]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB_PATH


def _library_flags():
    """the flag list build_library() compiles the product's units with"""
    return [f for f in HIPCC_FLAGS if f != "-shared"] + os.environ.get("WOST_HIPCC_DEFS", "").split()


PROBE_DIR = os.path.join(_HERE, "..", "tests", "probe")
PROBE_SRC = os.path.join(PROBE_DIR, "wost_probe.hip")
# (object, source) of the probe library: its own two units, and the product's csrc/wost_order.hip compiled a second time -- the
# order probe runs the product's key kernels and sort, it restates none of them
PROBE_UNITS = [("wost_probe.o", PROBE_SRC),
               ("wost_order_probe.o", os.path.join(PROBE_DIR, "wost_order_probe.hip")),
               ("probe_wost_order.o", os.path.join(CSRC, "wost_order.hip"))]
PROBE_PATH = os.path.join(LIB_DIR, "libwost_probe.so")


def build_probe(force=False, verbose=False):
    """libwost_probe.so (test infrastructure, tests/probe/): one elementwise kernel over the inline math functions of csrc/
    (wost_probe.hip) and a driver of the walk orders (wost_order_probe.hip, linked with csrc/wost_order.hip), every unit
    compiled with exactly the flags of the product's units -- it tests what those flags make of the product's code -- and
    rebuilt when the unit, a header of csrc/ or the flags change."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")]
    flags = _library_flags()
    stamp = os.path.join(OBJ_DIR, "probe_flags.stamp")
    flag_id = hashlib.sha256(" ".join(flags).encode()).hexdigest()
    try:
        same_flags = open(stamp).read().strip() == flag_id
    except OSError:
        same_flags = False
    jobs, objs = [], []
    for name, src in PROBE_UNITS:
        obj = os.path.join(OBJ_DIR, name)
        objs.append(obj)
        if force or not same_flags or _stale(obj, [src] + headers):
            cmd = [_hipcc()] + flags + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd)))
    # (as in build_library: every compiler is waited for before a failure is reported)
    failed = [(cmd, p.returncode) for cmd, p in jobs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(failed[0][1], failed[0][0])
    if jobs or not same_flags:
        with open(stamp, "w") as f:
            f.write(flag_id + "\n")
    if force or jobs or _stale(PROBE_PATH, objs):
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", PROBE_PATH]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return PROBE_PATH


def source_id():
    """identity of the kernel sources (csrc/*.h, *.hip, *.cpp and include/wost.h): committed counter files carry the id of
    the tree they were measured on, and bench.py marks them stale when the running tree differs"""
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp")))
    for f in files + [os.path.join(_HERE, "..", "include", "wost.h")]:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


HOST_DIR = os.path.join(_HERE, "host")
HOST_SOURCES = ["main.cpp", "exec.cpp", os.path.join("core", "problem.cpp"),
                os.path.join("integrator", "common.cpp"), os.path.join("integrator", "uniform", "integrator.cpp"),
                os.path.join("integrator", "guided", "integrator.cpp"), os.path.join("util", "json.cpp"),
                os.path.join("util", "image_io.cpp")]


def build_host(force=False, verbose=False):
    """elaina-exec: the C++ host mirror of the reference's entry point, linked against
    libwost_hip.so (rpath = $ORIGIN, both live in elaina_amd/lib)."""
    build_library(force=force, verbose=verbose)
    srcs = [os.path.join(HOST_DIR, s) for s in HOST_SOURCES]
    deps = list(srcs)
    for root, _, files in os.walk(HOST_DIR):
        deps += [os.path.join(root, f) for f in files if f.endswith(".h")]
    deps.append(LIB_PATH)
    if force or _stale(HOST_EXE, deps):
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I", HOST_DIR] + srcs + [
            "-L", LIB_DIR, "-lwost_hip", "-Wl,-rpath,$ORIGIN", "-o", HOST_EXE]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return HOST_EXE


if __name__ == "__main__":
    print(build_host(force=True, verbose=True))
    print(build_library(force=True, verbose=True))
    print(build_probe(force=True, verbose=True))
