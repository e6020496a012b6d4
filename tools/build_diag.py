"""Builds a DIAGNOSTIC libpdse (never the product library) with extra compile-time switches:

    python tools/build_diag.py -o /tmp/libpdse_diag.so -DPDSE_DIAG                    # the trace / ablation environment hooks
    python tools/build_diag.py -o /tmp/libpdse_slots.so -DBGLU_DIAG -DBGLU_SLOTSTAMP  # the block kernel's per-slot clock stamps
    PDSE_LIB=/tmp/libpdse_slots.so python tools/time_bglu.py

(-DBGLU_NO_MM / NO_REQ / ...: the block kernel's timing ablations, README.md.)"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    args = sys.argv[1:]
    out = args[args.index("-o") + 1]
    extra = [a for a in args if a.startswith("-D")]
    bdir = out + ".build"
    os.makedirs(bdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wno-pass-failed", "-I" + os.path.join(ROOT, "include"), "-I" + ge.CSRC] + extra

    def cc(src):
        obj = os.path.join(bdir, src.replace(".hip", ".o"))
        subprocess.run([hipcc] + flags + ["-c", os.path.join(ge.CSRC, src), "-o", obj], check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(ge.SOURCES), os.cpu_count() or 1)) as ex:
        objs = list(ex.map(cc, ge.SOURCES))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs, check=True)
    print("built", out, "with", " ".join(extra))


if __name__ == "__main__":
    main()
