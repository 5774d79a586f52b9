"""TEST INFRASTRUCTURE: compile the unmodified HIP sources for the host CPU against the
fiber-based HIP emulator (tests/hipemu/hip/hip_runtime.h) -> tests/hipemu/libfdtd_emu.so."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
CSRC = os.path.join(ROOT, "tidy3d_amd", "csrc")
LIB = os.path.join(HERE, "libfdtd_emu.so")
# every .hip and .hpp under csrc/ (a header added there is picked up without an edit here), and the files outside it
DEPS = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))) + [
    os.path.join(ROOT, "include", "fdtd_hip.h"), os.path.join(HERE, "hip_emu.cpp"),
    os.path.join(HERE, "hip", "hip_runtime.h"), os.path.join(HERE, "rccl", "rccl.h"),
    os.path.abspath(__file__)]


def hip_sources() -> list:
    """The library's translation units: the list the device build keeps (tidy3d_amd/build.py SOURCES), read from the file so that
    this script needs neither the package on sys.path nor its imports."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_fdtd_device_build", os.path.join(ROOT, "tidy3d_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.SOURCES)


def build(force: bool = False) -> str:
    if not force and os.path.exists(LIB) and all(
            os.path.getmtime(d) <= os.path.getmtime(LIB) for d in DEPS):
        return LIB
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++") or shutil.which("g++")
    # one object per translation unit, compiled side by side (the emulated library is rebuilt on every kernel edit: 4 min in one
    # compiler invocation, ~1.5 min this way), into a private directory so that two builds at once do not race
    import tempfile
    flags = [cxx, "-O2", "-g", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-I" + HERE,
             "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-pass-failed"]
    srcs = [*hip_sources(), os.path.join(HERE, "hip_emu.cpp")]
    tmp = tempfile.mkdtemp(prefix="fdtd_emu_")
    try:
        procs, objs = [], []
        for src in srcs:
            obj = os.path.join(tmp, os.path.basename(src) + ".o")
            cmd = [*flags, "-x", "c++", "-c", src, "-o", obj]
            print(" ".join(cmd), flush=True)
            procs.append((cmd, subprocess.Popen(cmd)))
            objs.append(obj)
        for cmd, pr in procs:
            if pr.wait() != 0:
                for _, other in procs:
                    if other.poll() is None:
                        other.kill()
                raise subprocess.CalledProcessError(pr.returncode, cmd)
        out = os.path.join(tmp, "libfdtd_emu.so")
        cmd = [cxx, "-shared", "-fPIC", "-Wl,-Bsymbolic", *objs, "-o", out]
        print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        shutil.move(out, LIB)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
