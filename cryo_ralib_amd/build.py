"""Builds libralign_hip.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc: one object per csrc/*.hip, compiled side by side,
then one link.  `python -m cryo_ralib_amd.build [-o OUT] [-DNAME[=VALUE] ...]` builds a variant (profiling switches) elsewhere."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libralign_hip.so")
CSRC = os.path.join(HERE, "csrc")
SOURCES = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + \
          [os.path.join(ROOT, "include", "ralign.h")]
MAX_JOBS = 16       # compiles at a time


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP alignment engine cannot be built")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(f) > t for f in SOURCES + HEADERS)


def build_hip(force=False, verbose=False, out=LIB, defines=()):
    """out: the library's path; defines: extra -D flags ("NAME" or "NAME=VALUE").  Any source or header newer than the default
    library rebuilds everything; another `out` or any define always builds."""
    if not force and out == LIB and not defines and not needs_build():
        return LIB
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include")] + ["-D" + d for d in defines]
    objdir = os.path.join(ROOT, "build", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    objs = [os.path.join(objdir, os.path.splitext(os.path.basename(s))[0] + ".o") for s in SOURCES]

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(min(MAX_JOBS, len(SOURCES))) as pool:
        list(pool.map(lambda so: run([hipcc_path()] + flags + ["-c", so[0], "-o", so[1]]), zip(SOURCES, objs)))
    run([hipcc_path(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + objs)
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    out = os.path.abspath(args[args.index("-o") + 1]) if "-o" in args else LIB
    print(build_hip(force=True, verbose=True, out=out, defines=[a[2:] for a in args if a.startswith("-D")]))
