"""Builds lib/libcova_hip.so (gfx950) from csrc/*.hip with hipcc -- in-tree, no JIT cache."""
import glob
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libcova_hip.so")
SOURCES = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.hip")))
HEADERS = sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.h")))


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(s) > t for s in SOURCES + HEADERS)


# per-file extra flags.  conv_wgrad4: no SLP vectorisation -- on gfx950 packed f32 VALU ops cannot issue in the shadow
# of an MFMA (LLVM unpacks them again and leaves the shuffle moves behind: 210 register moves per K-step of the input role).
FILE_FLAGS = {"conv_wgrad4.hip": ["-fno-slp-vectorize"]}


def flags(name=None):
    """hipcc's flags for the translation unit `name` (its FILE_FLAGS included); every build of a csrc file starts from these.
    -Werror=missing-prototypes: common.h includes include/cova_hip.h, so a COVA_API definition that the header does not
    declare stops the build (one that disagrees with its declaration is a "conflicting types" error under any flags)."""
    return (["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
             "-Werror=missing-prototypes"] + FILE_FLAGS.get(os.path.basename(name) if name else None, []))


def build(force=False, verbose=False):
    if not force and not needs_build():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    objdir = os.path.join(PKG_DIR, "lib", "obj")
    os.makedirs(objdir, exist_ok=True)
    extra = os.environ.get("COVA_EXTRA_FLAGS", "").split()
    procs, objs = [], []
    for src in SOURCES:                        # one hipcc per translation unit, in parallel
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        cmd = [hipcc] + flags(src) + extra + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB_PATH]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
